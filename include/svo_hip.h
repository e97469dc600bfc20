/*
 * svo_hip.h — C ABI of libsvo_hip.so, the MI355X (gfx950) implementation of the
 * stereo-SVO hot path. No torch / OpenCV / C++ types cross this boundary.
 *
 * The reference library (libstereosvo.so) has no C ABI: its consumers link
 * mangled C++ symbols (src/app/Makefile:17-18, src/python/setup.py:29-33).
 * Each entry point below names the reference interface it replaces; the C++
 * facade in stereo-svo-slam_amd/hostcpp/ and INTEGRATION.md show the binding a
 * maintainer of the reference would add.
 *
 * Conventions: every function returns 0 on success, < 0 on error
 * (svo_last_error() has the text); nothing throws. Unless stated otherwise
 * all data pointers are DEVICE pointers and work is enqueued on the handle's
 * HIP stream without synchronising.
 */
#ifndef SVO_HIP_H
#define SVO_HIP_H

#include <stddef.h>

#include "svo_types.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SVO_OK = 0,
    SVO_ERR_INVALID = -1,
    SVO_ERR_HIP = -2,
    SVO_ERR_NO_DEVICE = -3,
    SVO_ERR_CAPACITY = -4
};

typedef struct svo_handle svo_handle;

const char *svo_last_error(void);
int svo_version(void);

/* one handle per (GPU, caller thread): stream + small workspaces */
int svo_handle_create(int device, int max_keypoints, svo_handle **out);
int svo_handle_destroy(svo_handle *h);
int svo_handle_set_stream(svo_handle *h, void *hip_stream); /* hipStream_t, NULL = default */
int svo_handle_synchronize(svo_handle *h);
/* The two Gauss-Newton kernels (sparse alignment, reprojection) have two forms of the normal
 * equations. Default (fast_solver = 0): the reference's arithmetic — `hessian += row^T row`,
 * `residual -= row * diff` accumulated row by row in storage order and the Jacobi-SVD
 * pseudo-inverse of Matx66f::inv(DECOMP_SVD) (src/lib/pose_estimator.cpp:399-405,472-477,
 * pose_refinement.cpp:393-398): poses, costs and iteration traces are the CPU restatement's, bit
 * for bit. fast_solver = 1: J^T (sum g g^T) J per keypoint summed in a tree and an LDL^T solve in
 * double (SVD only for rank deficient systems): ~1.5x the frame rate, same minimum within
 * 1e-4 m / rad on smooth motion, but not the reference's iteration trace.
 * (The cost is summed in the reference's order in both.) */
int svo_handle_set_fast_solver(svo_handle *h, int on);
int svo_handle_set_exact_pinv(svo_handle *h, int on);   /* older name: set_fast_solver(!on) */

/* device memory for callers without a HIP toolchain (the C++ facades in
 * stereo-svo-slam_amd/hostcpp/, ctypes): plain hipMalloc / hipFree and copies that are
 * ordered on the handle's stream and complete on return */
int svo_device_malloc(size_t bytes, void **out);
int svo_device_free(void *p);
int svo_copy_to_device(svo_handle *h, void *dst, const void *src, size_t bytes);
int svo_copy_to_host(svo_handle *h, void *dst, const void *src, size_t bytes);
/* rows of `width` bytes: host image (src_stride) -> device image (dst_stride) */
int svo_copy_image_to_device(svo_handle *h, void *dst, size_t dst_stride, const void *src,
                             size_t src_stride, size_t width, size_t height);

/* ---- stage level entry points (one per row of SURVEY §8a) ----------------
 * P1  createImgPyramid / halfSample          src/lib/stereo_slam.cpp:93-121
 * levels[0] = input; levels[1..n-1].data = caller-allocated outputs
 * (width/height/stride are filled in; stride = width). */
int svo_build_pyramid(svo_handle *h, int n_levels, svo_image *levels);
/* P2  image part of cv::buildOpticalFlowPyramid(.., Size(win,win), 2)
 *                                              src/lib/stereo_slam.cpp:137-139
 * levels[l>=1] receive pyrDown of the previous level; *n_out = usable levels. */
int svo_build_lk_pyramid(svo_handle *h, int max_levels, int win, svo_image *levels, int *n_out);

/* R   cv::remap(src, dst, map_x, map_y, INTER_LINEAR), BORDER_CONSTANT 0   src/app/euroc_input.cpp:69-70
 * n images that share one map: src[i] (any size) -> dst[i] (dst width x height = the map's size, same for all i);
 * map_x / map_y: device, dst width x height floats, dense rows. Bit-exact to OpenCV's fixed-point remap
 * (INTER_BITS 5: positions rounded half to even to 1/32 pixel, 15-bit weights; a map entry that is not
 * finite or whose |value * 32| >= 2^31 gives 0). Sources up to 16383 pixels a side. */
int svo_remap_linear(svo_handle *h, int n, const svo_image *src, svo_image *dst,
                     const float *map_x, const float *map_y);

/* R'  the same remap with a map per image (camera rigs): n_maps maps of one size (map_x[m] / map_y[m]: device, dst width x
 * height floats, dense rows; host arrays of pointers), image i through map map_of_image[i] in [0, n_maps), in any order;
 * a map that no image uses is allowed (it is checked, not read). The arithmetic is svo_remap_linear's. The images are
 * sorted by map, and images that share a map share its loads as in svo_remap_linear. SVO_ERR_INVALID: n_maps < 1, an
 * index out of range, a NULL map, dst images of mixed sizes; the handle stays usable. */
int svo_remap_linear_multi(svo_handle *h, int n, const svo_image *src, svo_image *dst, int n_maps,
                           const float *const *map_x, const float *const *map_y, const int *map_of_image);

/* M   cv::initUndistortRectifyMap(K, D, R, P, size, CV_32F, map_x, map_y)   src/app/euroc_input.cpp:24-49
 * One camera's calibration as EurocInput reads it from the settings file: K, R row-major 3x3, P the left 3x3 of the
 * file's 3x4 projection, D = k1, k2, p1, p2, k3, k4, k5, k6 (zeros where the model has fewer). The maps are plain
 * IEEE binary64 arithmetic, every operation rounded on its own (no fused multiply-add), in exactly this association:
 *   M[r][c] = (P[r][0]*R[0][c] + P[r][1]*R[1][c]) + P[r][2]*R[2][c];   a..i = M row-major
 *   c00 = e*i - f*h;  c01 = f*g - d*i;  c02 = d*h - e*g;  det = (a*c00 + b*c01) + c*c02;  t = 1.0/det
 *   ir = { c00*t, (c*h-b*i)*t, (b*f-c*e)*t,  c01*t, (a*i-c*g)*t, (c*d-a*f)*t,  c02*t, (b*g-a*h)*t, (a*e-b*d)*t }
 *   pixel (column j, row i):  X = j*ir[0] + (i*ir[1] + ir[2]);  Y = j*ir[3] + (i*ir[4] + ir[5]);
 *                             W = j*ir[6] + (i*ir[7] + ir[8]);  iw = 1.0/W;  x = X*iw;  y = Y*iw
 *   x2 = x*x;  y2 = y*y;  r2 = x2 + y2;  _2xy = (2*x)*y
 *   kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2)
 *   xd = (x*kr + p1*_2xy) + p2*(r2 + 2*x2);   yd = (y*kr + p1*(r2 + 2*y2)) + p2*_2xy
 *   map_x = (float)(K[0]*xd + K[2]);  map_y = (float)(K[4]*yd + K[5])        (round to nearest even)
 * Values that are not finite propagate as IEEE says (W = 0 on a horizon line); the remap treats them as outside.
 * (OpenCV's scalar loop accumulates X += ir[0] along a row, its AVX2 path does not: this direct form is the
 * library's statement; on the EuRoC calibrations at 752 x 480 all three give the same float bits.) */
typedef struct svo_camera_calibration {   /* 280 bytes: K at 0, D at 72, R at 136, P at 208 */
    double K[9], D[8], R[9], P[9];
} svo_camera_calibration;
/* ir of the statement above; host only (works without a GPU). The one place that validates a calibration, used by
 * every entry that takes one: SVO_ERR_INVALID (ir untouched) when an input is not finite or det is 0 or not finite. */
int svo_rectify_inverse(const svo_camera_calibration *cal, double ir[9]);
/* the maps of n cameras (cal: host array) in ONE launch: map_x[c] / map_y[c] (host arrays of device pointers) receive
 * width x height floats each, dense rows; any width, height >= 1. A calibration svo_rectify_inverse rejects, a NULL
 * plane, n < 0, or 2^23 or more (64 x 64 tile, camera) pairs: SVO_ERR_INVALID, nothing launched. */
int svo_build_rectify_maps(svo_handle *h, int n, const svo_camera_calibration *cal, int width, int height,
                           float *const *map_x, float *const *map_y);

/* I   the per-pixel step of the reference's ImageInput classes before StereoSlam::new_image: cvtColor(BGR2GRAY)
 *     and the halves of a side-by-side frame (src/app/video_input.cpp:29-36), extractChannel of a 3-channel
 *     frame (src/app/econ_input.cpp:102-103). The arithmetic:
 *       gray  Y = (3735 B + 19235 G + 9798 R + 2^14) >> 15   (OpenCV 4.x RGB2Gray<uchar>: 15-bit weights, CV_DESCALE)
 *       channel extract: byte k of an interleaved 3-channel pixel
 *       side by side, output width W: right = columns 0 .. W-1, left = columns W .. 2W-1 of the frame
 * An input format says how the buffers of one sequence become its left and right 8-bit images. */
enum { SVO_INPUT_GRAY_PAIR = 0,   /* default: left[s], right[s] are two 8-bit images                                 */
       SVO_INPUT_BGR_PAIR  = 1,   /* two 3-channel images, B,G,R order                                               */
       SVO_INPUT_RGB_PAIR  = 2,   /* ... R,G,B order                                                                 */
       SVO_INPUT_SBS_GRAY  = 3,   /* ONE buffer per sequence, >= 2W pixels per row: right = left half, left = right half */
       SVO_INPUT_SBS_BGR   = 4,
       SVO_INPUT_SBS_RGB   = 5,
       SVO_INPUT_CH3_ECON  = 6 }; /* ONE W x H x 3 buffer: right = channel 1, left = channel 2                      */
enum { SVO_INGEST_COPY = 0,       /* the output byte is byte `channel` of the source pixel                           */
       SVO_INGEST_GRAY = 1 };     /* (weight[0] c0 + weight[1] c1 + weight[2] c2 + 2^14) >> 15 of its three bytes     */
typedef struct svo_input_side {
    int32_t buffer;             /* which buffer of the sequence: 0 = left[s] (src_a), 1 = right[s] (src_b)          */
    int32_t start_column;       /* column of the buffer that becomes column 0 of the image                          */
    int32_t op, channel;        /* SVO_INGEST_*                                                                      */
    int32_t weight[3];
} svo_input_side;
typedef struct svo_input_layout {
    int32_t buffers;            /* per sequence: 1 or 2                                                              */
    int32_t channels;           /* bytes per pixel: 1 or 3                                                           */
    int32_t min_row_pixels;     /* pixels a buffer row holds at least (its stride: >= min_row_pixels * channels)     */
    svo_input_side left, right;
} svo_input_layout;
/* the layout of `format` for images of `width` pixels; needs no GPU. Unknown format or width < 1: SVO_ERR_INVALID */
int svo_input_format_info(int format, int width, svo_input_layout *out);
/* n buffers src_a[i] (and src_b[i] for the pair formats; otherwise src_b is ignored and may be NULL) into n left
 * and n right 8-bit images. Every left[i] / right[i] has the size of left[0] (W x H, any W, H >= 1, stride >= W);
 * a source has at least min_row_pixels x H pixels of `channels` bytes (svo_image.width / height in pixels, stride in
 * bytes >= width * channels). Any base address and stride: rows that are dword aligned (source) and 16-byte
 * aligned (output) take the wide path, the rest goes byte by byte; nothing outside the rows given is read or written. */
int svo_convert_frames(svo_handle *h, int format, int n, const svo_image *src_a, const svo_image *src_b,
                       svo_image *left, svo_image *right);

/* A   PoseEstimator::estimate_pose(guess, out) src/include/pose_estimator.hpp:19-27,
 *                                              src/lib/pose_estimator.cpp:115-130
 * prev_pyr/cur_pyr: cam->max_pyramid_levels halfSample levels (host array of
 * views onto device memory). pose_guess/pose_out/cost/trace: device memory;
 * trace = [SVO_MAX_PYRAMID_LEVELS] svo_gn_trace or NULL.
 * dbg (optional, device, 48 floats): H, b, step of the first get_gradient on dbg_level.
 * One departure from the reference: a keypoint whose Jacobian has an entry that is not finite (a point in the
 * camera plane of the pose) takes no part in H and b. The reference does the same while none of its patch pixels
 * passes the gradient bounds, and otherwise returns NaN. */
int svo_sparse_align(svo_handle *h, const svo_image *prev_pyr, const svo_image *cur_pyr,
                     const svo_kp2d *kps2d, const svo_kp3d *kps3d, const uint32_t *flags, int n,
                     const svo_camera_settings *cam, const float *pose_guess, float *pose_out,
                     float *cost, svo_gn_trace *trace, float *dbg, int dbg_level);

/* A3  project_keypoints(pose, in, camera_settings, out)   src/include/transform_keypoints.hpp:17-19,
 *                                              src/lib/transform_keypoints.cpp:11-48
 * pose: 6 floats in device memory. */
int svo_project_keypoints(svo_handle *h, const float *pose, const svo_kp3d *kps3d, int n,
                          const svo_camera_settings *cam, svo_kp2d *out);

/* B2  OpticalFlow::calculate_optical_flow      src/include/optical_flow.hpp:26-30,
 *                                              src/lib/optical_flow.cpp:14-56 */
int svo_klt_track(svo_handle *h, const svo_image *prev_lk, const svo_image *cur_lk, int n_levels,
                  const svo_kp2d *prev_pts, svo_kp2d *cur_pts, int n, int win,
                  uint8_t *status, float *err);

/* B1+B3  merge of PoseRefiner::refine_pose + PoseRefiner::update_pose
 *                                              src/lib/pose_refinement.cpp:125-150,236-290
 * tracked/err may be NULL (no merge). */
int svo_reproj_gn(svo_handle *h, svo_kp2d *kps2d, const svo_kp3d *kps3d, uint32_t *flags, int n,
                  const svo_camera_settings *cam, const svo_kp2d *tracked, const float *err,
                  const float *pose_in, float *pose_out, float *cost, svo_gn_trace *trace);

/* C1  DepthFilter::calculate_disparities       src/lib/depth_filter.cpp:259-327
 *     (clamp_half = 0: the loop of DepthCalculator::calculate_depth,
 *      src/lib/depth_calculator.cpp:200-240) */
int svo_ssd_disparity(svo_handle *h, const svo_image *left, const svo_image *right,
                      const svo_kp2d *kps2d, int n, int win, int search_x, int search_y,
                      int clamp_half, float *disparity);

/* C2+D1  DepthFilter::outlier_check + update_kps3d
 *                                              src/lib/depth_filter.cpp:52-128,130-257
 * ref3d/ref2d = keyframe->kps.kps3d/kps2d[keypoint_index], kf_pose = n*6 floats. */
int svo_depth_filter_update(svo_handle *h, const svo_kp2d *kps2d, svo_kp3d *kps3d,
                            const uint32_t *flags, int n, const svo_camera_settings *cam,
                            const float *frame_pose, const float *disparity,
                            const svo_kp3d *ref3d, const svo_kp2d *ref2d, const float *kf_pose,
                            int32_t *outlier_count, int32_t *inlier_count,
                            float *kf_inv_depth, float *kf_variance,
                            int do_outlier_check, int do_update);

/* F2  CornerDetector::detect_keypoints and detect_keypoints_on_each_level
 *                                              src/lib/corner_detector.cpp:13-79,
 *                                              src/lib/depth_calculator.cpp:11-35
 * One keypoint per grid cell on each of n_levels images (1..SVO_MAX_PYRAMID_LEVELS; host array of views
 * onto device memory: any width, height, stride >= width and base address); level l uses cells of
 * (grid_width >> l) x (grid_height >> l). The launch is the tracker's (same kernel shape, same argument
 * block). cells[l * max_cells + c] (device) receives cell c of level l, cells in row-major order;
 * counts[l] (device, n_levels ints) the level's cell count: (width / cell width) * (height / cell height).
 * max_cells >= every level's cell count (svo_detect_shape has the tracker's value for halved levels).
 * SVO_ERR_INVALID for what has no value in the reference: a level-0 cell outside 4..96 x 4..64
 * (svo_ctx_create rejects it too), a level whose shifted cell size is 0 (the reference's cell loop does
 * not end) or whose height is below its cell height (the reference reads past the last row). */
typedef struct svo_det_cell {
    float   x, y;               /* pixel of the level                                              */
    float   score;              /* FAST score or saturated Sobel dx response                       */
    int32_t type;               /* SVO_KP_FAST / SVO_KP_EDGELET                                    */
} svo_det_cell;
int svo_detect_keypoints(svo_handle *h, int n_levels, const svo_image *levels, int grid_width,
                         int grid_height, int max_cells, svo_det_cell *cells, int32_t *counts);
/* the shape such a launch runs, without a GPU, for levels that halve from width x height (level l:
 * width >> l, height >> l): *max_cells = the largest cell count of a level (at least 1: the tracker's
 * value), *cell_width / *cell_height = the largest cell of the kernel shape chosen, *list_capacity = the
 * FAST corners of one cell + 1 px that the shape keeps for its score pass (more are scored where they are
 * found). Any out pointer may be NULL. Same SVO_ERR_INVALID cases as svo_detect_keypoints. */
int svo_detect_shape(int width, int height, int n_levels, int grid_width, int grid_height,
                     int *max_cells, int *cell_width, int *cell_height, int *list_capacity);

/* ---- whole tracker: StereoSlam (src/include/stereo_slam.hpp:27-79) --------
 * One svo_ctx owns `n_sequences` independent StereoSlam instances; the sequences of
 * a group share every kernel launch (sequence = a grid dimension);
 * n_sequences = 1 is the drop-in for one StereoSlam object. A ctx is
 * single-caller; different ctxs are independent (own stream, own counters —
 * the reference's process-global keyframe counters, keyframe_manager.cpp:8 and
 * depth_calculator.cpp:135, are per sequence here). */
typedef struct svo_ctx svo_ctx;

/* SVO_MEM_DEVICE_BORROW: device images that the ctx uses IN PLACE as level 0 of its pyramids and
 * as the right image — no copy, like the reference, whose level 0 is a shallow alias of the caller's
 * cv::Mat (src/lib/stereo_slam.cpp:115). The caller keeps every image valid and unchanged while a
 * frame or keyframe of the ctx refers to it: until its sequence ends. Once svo_ctx_restart_sequences
 * has been processed for a slot (after svo_wait) no frame of the ended sequence is read again and the
 * caller may reuse or free them; otherwise until svo_ctx_destroy. With
 * rectification on (svo_ctx_set_rectification) or an input format that converts (svo_ctx_set_input_format: every one
 * but GRAY_PAIR and SBS_GRAY) the buffers are only read during their step and level 0 is the ctx's own image: they may
 * be reused after svo_wait. SVO_INPUT_SBS_GRAY without rectification uses the two halves of the frame in place
 * (nothing is converted or copied): the lifetime rule above holds for the frame. */
enum { SVO_MEM_HOST = 0, SVO_MEM_DEVICE = 1, SVO_MEM_DEVICE_BORROW = 2 };

/* StereoSlam::StereoSlam(const CameraSettings&)         src/lib/stereo_slam.cpp:29-41 */
int svo_ctx_create(const svo_camera_settings *cam, int width, int height, int n_sequences,
                   int device, svo_ctx **out);
int svo_ctx_destroy(svo_ctx *ctx);

/* StereoSlam::new_image(left, right, time_stamp)        src/lib/stereo_slam.cpp:123-271
 * for every sequence of the ctx: left[s]/right[s] point to 8-bit images of the
 * ctx size with `stride` bytes per row, in host (SVO_MEM_HOST) or device memory.
 * The images are copied; the caller may reuse its buffers on return. Returns
 * after the frame is complete (like the reference). A sequence whose two pointers are
 * NULL sits the step out with its state untouched (sequences of one ctx may have different
 * lengths). Every slot of a fresh ctx is EMPTY: a slot starts its sequence with the first frame
 * it is given, at whatever step (see svo_ctx_restart_sequences). */
int svo_new_images(svo_ctx *ctx, const uint8_t *const *left, const uint8_t *const *right,
                   int stride, const float *time_stamps, int mem);
/* Pipelined form (no counterpart in the reference, whose new_image is synchronous): svo_submit_images() queues one frame set (same arguments; the images,
 * host or device, must stay valid until svo_wait) on every sequence group and returns; svo_wait()
 * blocks until all queued frame sets are processed and reports the first error. The groups
 * (svo_ctx_get_groups; SVO_GROUPS overrides the default) advance independently, each on its
 * own HIP stream and host thread, so one group's host round trips (keyframe decision,
 * argument blocks) overlap the other groups' kernels. svo_new_images = submit + wait; every
 * getter waits first. */
int svo_submit_images(svo_ctx *ctx, const uint8_t *const *left, const uint8_t *const *right,
                      int stride, const float *time_stamps, int mem);
int svo_wait(svo_ctx *ctx);
int svo_ctx_get_groups(svo_ctx *ctx, int *n_groups);
/* Sequence lifecycle (the reference's user constructs a new StereoSlam per sequence, src/app/main.cpp).
 * The named slots end their current sequence. Ordered with the frame sets: it takes effect after every
 * frame set submitted before it and before every one submitted after it; it does not wait. From then
 * on a slot is EMPTY: NULL images keep it empty, and the next frame it is given is frame 0 of a new
 * sequence, exactly like the first frame of a fresh ctx (zero pose, keyframe 0 from that frame, new
 * pose filter, frame_id 0, keyframe ids from 0, colour LCG reseeded, empty trajectory). The getters
 * describe the slot's current run; on an empty slot they return what a fresh ctx returns. Ending a
 * sequence gives its image sets and keyframe storage back to the ctx (svo_ctx_get_memory), so a slot
 * can run any number of sequences in bounded memory.
 * An empty slot named here is left alone. Bad index: SVO_ERR_INVALID, nothing queued. A failed ctx
 * rejects it like svo_submit_images. */
int svo_ctx_restart_sequences(svo_ctx *ctx, const int *seqs, int n);
/* When a restart ends a non-empty run, the ctx keeps a host record of it (24 B per frame for the
 * trajectory) until svo_drop_finished_runs. Like every getter these wait for the queues. */
typedef struct svo_run_info {
    int32_t seq, run;           /* slot, and the ordinal of the run in that slot (0, 1, ...)        */
    int32_t frames, keyframes;
    float   last_time_stamp;
    float   pose[6];            /* final filtered pose                                              */
} svo_run_info;
/* *n = kept records of the slot, oldest first */
int svo_get_finished_runs(svo_ctx *ctx, int seq, int *n);
/* record i of the slot; copies min(*n_poses, cap) poses of its trajectory. info / trajectory / n_poses may be NULL */
int svo_get_finished_run(svo_ctx *ctx, int seq, int i, svo_run_info *info, svo_pose *trajectory,
                         int cap, int *n_poses);
/* forgets the records of the slot; seq < 0: of every slot */
int svo_drop_finished_runs(svo_ctx *ctx, int seq);
/* device memory of the ctx. Image sets and keyframe slabs are allocated in chunks when a free list runs dry and
 * return to it when a keyframe's images are retired or a sequence ends. */
typedef struct svo_memory {
    int64_t device_bytes;       /* every device allocation of the ctx's groups                      */
    int64_t klt_cache_bytes;    /* of which the KLT template cache                                  */
    int32_t image_sets, image_sets_free;          /* pyramids of one frame: made so far / not in use */
    int32_t keyframe_slabs, keyframe_slabs_free;  /* keypoint storage of one keyframe                */
} svo_memory;
int svo_ctx_get_memory(svo_ctx *ctx, svo_memory *out);
/* ---- trimming: a sequence that runs without end -------------------------------------------------------------------
 * A keyframe is RETIRED once no keypoint of the current frame originates from it (its image set goes back then). Its
 * points are final from there on: neither the tracker nor the depth filter touches it again, the keypoints of every
 * later frame have an origin id at or above the retired count, and write-back goes to origin keyframes only. A
 * retired keyframe still holds its keypoint storage (15 dwords per keypoint of capacity) and a record of the slot's
 * keyframe table, which has room for `table` RESIDENT keyframes (4096; the diagnostic SVO_KEYFRAME_TABLE, a power of
 * two 4 .. 4096, makes it smaller; a bad value: the default). Trimming drops a prefix of the retired keyframes: their
 * storage returns to the ctx (svo_memory.keyframe_slabs_free) and their table records become free for new keyframes.
 * It cannot change any frame. Ids never move: keyframe ids, svo_get_keyframe_count, svo_run_info.keyframes and the
 * keypoints' keyframe_id stay absolute and keep counting up; the resident keyframes of a slot are [first, count), with
 * first <= retired <= count - 1, and a new keyframe fails with SVO_ERR_CAPACITY only when count - first == table.
 * A restart, the end of a sequence and a load free the resident keyframes; first returns to 0 with the ids.
 * Not trimmed: the host trajectory, 24 B per frame and slot (about 1.7 MB per hour and slot at 20 Hz).
 *
 * svo_submit_trim_keyframes: each named slot drops its keyframes with id < min(below[i], retired) as of when the job
 * runs (below == NULL: everything retired; seqs == NULL names every slot in order, n is ignored). Queued exactly like
 * a restart: behind every frame set, restart, load and export submitted before it and ahead of what follows; it does
 * not wait, and only the groups that own a named slot get work. Nothing to drop, or an empty slot, is not an error.
 * Host bookkeeping only: no launch, no copy. Rejected with SVO_ERR_INVALID and nothing queued: a slot out of range or
 * named twice; a failed ctx, as in svo_submit_images. */
int svo_submit_trim_keyframes(svo_ctx *ctx, const int *seqs, const int *below, int n);
int svo_trim_keyframes(svo_ctx *ctx, const int *seqs, const int *below, int n);   /* submit + wait */
/* keep = -1 (the default): a slot never trims on its own. keep >= 0: after each step a slot with retired - first >
 * keep is trimmed to first = retired - keep. A setter: waits for the queues. With SVO_KEEP_KEYFRAME_IMAGES=1 nothing
 * retires and so nothing is trimmed. keep < -1: SVO_ERR_INVALID. */
int svo_ctx_set_keyframe_window(svo_ctx *ctx, int keep);
typedef struct svo_keyframe_range {   /* 16 bytes */
    int32_t first;                    /* the oldest resident keyframe (0 until the slot is trimmed)                   */
    int32_t retired;                  /* keyframes below it are final and may be trimmed                              */
    int32_t count;                    /* svo_get_keyframe_count: ids [first, count) are resident                      */
    int32_t table;                    /* resident keyframes a slot can hold                                           */
} svo_keyframe_range;
/* a getter: waits for the queues. An empty slot: {0, 0, 0, table}. */
int svo_get_keyframe_range(svo_ctx *ctx, int seq, svo_keyframe_range *out);
/* EurocInput's rectification (maps :48-49, remap :69-70) inside the tracker: from the next frame on, the
 * images given to svo_new_image(s) / svo_submit_images are RAW images of the ctx size, remapped on the
 * device before the pyramids. left_* rectify the library's left image (the reference's M1r/M2r: cam1 with
 * RIGHT.*), right_* its right image (M1l/M2l). Each map: width x height floats, dense rows, host
 * (SVO_MEM_HOST) or device (SVO_MEM_DEVICE) memory; copied. All four NULL: off. Waits for queued frames.
 * The arithmetic is svo_remap_linear's. These are the maps of rig 0: every slot that is not bound to another rig
 * (svo_ctx_assign_rigs) shares them; they apply to every frame of those slots, keyframes and the first frame included. With
 * SVO_MEM_DEVICE_BORROW and rectification on, the raw frames are read once and level 0 is the ctx's own
 * rectified image: the caller may reuse the raw buffers once the step is done (after svo_wait). */
int svo_ctx_set_rectification(svo_ctx *ctx, const float *left_map_x, const float *left_map_y,
                              const float *right_map_x, const float *right_map_y, int mem);
/* ---- camera rigs: slots of one ctx with their own intrinsics and rectification maps ------------------------------
 * A rig is what differs between two units of one camera model: the ten float settings and, optionally, the four
 * rectification maps (all four or none; ctx size, dense rows, host or device memory: mem; copied, as in
 * svo_ctx_set_rectification). The integer settings, the image size and the input format stay the ctx's: they choose
 * launch shapes and storage. Rig 0 always exists: the settings given to svo_ctx_create and whatever
 * svo_ctx_set_rectification holds. Every slot starts bound to rig 0, and a ctx that never adds a rig behaves and
 * launches as one without this interface. The slots of a group still share every launch: the kernels read the
 * intrinsics from the slot's argument block, and the remap takes a map per image when the images of a step do not
 * share one (svo_remap_linear_multi's kernel; slots whose rig has no maps are used as given in the same step, in
 * place with SVO_MEM_DEVICE_BORROW: the lifetime rule above then holds per slot). A rig's maps take
 * 2 x (6 B per pixel of the 64-aligned ctx size) of device memory. Maps are not part of a snapshot. */
typedef struct svo_rig {            /* 80 bytes */
    float baseline, fx, fy, cx, cy, k1, k2, k3, p1, p2;   /* as in svo_camera_settings; finite, fx, fy > 0 */
    const float *left_map_x, *left_map_y, *right_map_x, *right_map_y;   /* all four or all NULL */
    int32_t mem;                    /* of the maps: SVO_MEM_HOST / SVO_MEM_DEVICE */
    int32_t _reserved;              /* 0 */
} svo_rig;
/* adds n rigs; ids[i] >= 1 receives the id of rigs[i]. Waits for queued work. A value that is not finite, fx or
 * fy <= 0, some but not all maps, a bad mem: SVO_ERR_INVALID, nothing added. */
int svo_ctx_add_rigs(svo_ctx *ctx, const svo_rig *rigs, int n, int *ids);
/* removes the named rigs and frees their maps. Waits for queued work. Rig 0, an unknown id, or a rig that a slot is
 * bound to: SVO_ERR_INVALID, nothing removed, the ctx carries on. */
int svo_ctx_remove_rigs(svo_ctx *ctx, const int *ids, int n);
/* binds slot seqs[i] to rig rigs[i]. Ordered with the frame sets exactly like svo_ctx_restart_sequences, and like it
 * it ends the slot's sequence if it has one (the run goes to the finished runs, its storage back to the free lists):
 * the slot's next frame is frame 0 of a new sequence under that rig, so a calibration never changes inside a
 * sequence. The binding survives later restarts. Does not wait. A bad slot or an unknown rig: SVO_ERR_INVALID,
 * nothing queued. A failed ctx rejects it like svo_submit_images. */
int svo_ctx_assign_rigs(svo_ctx *ctx, const int *seqs, const int *rigs, int n);
/* the rig the slot is bound to and the full settings it tracks with (either may be NULL). Waits like every getter. */
int svo_ctx_get_slot_rig(svo_ctx *ctx, int seq, int *rig, svo_camera_settings *cam);
/* *n = rigs of the ctx, rig 0 included; *map_bytes = device bytes of the maps of the added rigs (also counted in
 * svo_memory.device_bytes). Either may be NULL. Waits. */
int svo_ctx_get_rigs(svo_ctx *ctx, int *n, int64_t *map_bytes);
/* EurocInput's whole rectification set-up (src/app/euroc_input.cpp:24-49) inside the ctx: rigs whose maps come from
 * calibrations instead of float planes. rigs[i] carries the ten float settings as svo_ctx_add_rigs validates them;
 * its four map pointers must be NULL. left[i] / right[i]: the cameras behind the library's left / right image
 * (EurocInput: left <- RIGHT.*, right <- LEFT.*), validated by svo_rectify_inverse. One launch builds all 2n maps
 * straight in the remap kernels' fixed-point form (svo_build_rectify_maps' float -> remap_prep's entries, fused): no
 * float plane is allocated, uploaded or read, a rig costs its 2 x map bytes and nothing transient. The rigs are the
 * rigs svo_ctx_add_rigs makes from svo_build_rectify_maps' planes, byte for byte. Waits for queued work; every rig
 * is built before any is added: SVO_ERR_INVALID (map pointers set, a rejected calibration, n < 0, ...) adds nothing. */
int svo_ctx_add_rigs_calibrated(svo_ctx *ctx, const svo_rig *rigs, const svo_camera_calibration *left,
                                const svo_camera_calibration *right, int n, int *ids);
/* the same for rig 0, with svo_ctx_set_rectification's rules: both NULL turns rectification off; one NULL or a
 * rejected calibration: SVO_ERR_INVALID, the old maps stay. */
int svo_ctx_set_calibration(svo_ctx *ctx, const svo_camera_calibration *left, const svo_camera_calibration *right);
/* The input format of the frames given to svo_new_image(s) / svo_submit_images from the next frame on, for every
 * active slot (a slot's first frame and keyframes included); may be switched between frames. Waits for queued
 * frames. Default SVO_INPUT_GRAY_PAIR: with it no launch, copy or allocation is added. The formats with ONE buffer
 * per sequence take it in left[s]; right[s] (and the `right` array itself) is ignored and may be NULL; a NULL
 * left[s] sits the step out. `stride` is the buffer's row pitch in bytes (>= min_row_pixels * channels of
 * svo_input_format_info for the ctx width). svo_new_image follows the same rule: right and right_stride are ignored,
 * width and height stay the ctx's. All three memory modes work with every format; host buffers go through the
 * staging buffer (one slot per sequence for the one-buffer formats). With rectification also on the order is
 * format -> remap -> pyramids, as EurocInput would do on colour images. A bad format: SVO_ERR_INVALID, the ctx
 * keeps its setting. */
int svo_ctx_set_input_format(svo_ctx *ctx, int format);
/* n_sequences == 1, host memory: the exact shape of StereoSlam::new_image */
int svo_new_image(svo_ctx *ctx, const uint8_t *left, int left_stride, const uint8_t *right,
                  int right_stride, int width, int height, float time_stamp);

/* Frame::pose of the current frame (get_frame, src/lib/stereo_slam.cpp:278-284) */
int svo_get_pose(svo_ctx *ctx, int seq, float pose[6]);
/* Frame::kps of the current frame; returns the count in *n (copies min(n, cap)) */
int svo_get_frame_keypoints(svo_ctx *ctx, int seq, svo_kp2d *kps2d, svo_kp3d *kps3d,
                            svo_kp_info *info, int cap, int *n);
/* get_keyframes / get_keyframe (src/lib/stereo_slam.cpp:273-289). The count is the number of ids given out; an id
 * below svo_keyframe_range.first: SVO_ERR_INVALID, "keyframe %d was trimmed" */
int svo_get_keyframe_count(svo_ctx *ctx, int seq, int *count);
int svo_get_keyframe(svo_ctx *ctx, int seq, int id, svo_kp2d *kps2d, svo_kp3d *kps3d,
                     svo_kp_info *info, float pose[6], int cap, int *n);
/* get_trajectory (src/lib/stereo_slam.cpp:291-294) */
int svo_get_trajectory(svo_ctx *ctx, int seq, svo_pose *out, int cap, int *n);
/* StereoSlam::update_pose (12-state Kalman)             src/lib/stereo_slam.cpp:296-359
 * The one-slot form: waits for every queue of the ctx and runs the filter on the calling thread. On an empty or
 * restarted slot it works on a fresh filter. */
int svo_update_pose(svo_ctx *ctx, int seq, const float pose[6], const float speed[6],
                    const float pose_var[6], const float speed_var[6], double dt,
                    float filtered[6]);

/* ---- batched pose-filter updates: the IMU loop of many slots as one queued job per group -------------------------
 * The batched, queued form of svo_update_pose: counts[i] samples for slot seqs[i] (seqs == NULL: slot i, n is then
 * the ctx's slots; a count of 0 leaves the slot untouched). `samples` holds the samples of seqs[0] first, in the
 * order they are applied, then those of seqs[1], and so on. Every group that owns a named slot with a positive count
 * gets one entry in its queue, behind the frame sets, restarts, exports, saves and loads submitted so far; nothing
 * is waited for and no group waits for another. The group's worker applies the pending update of its last frame
 * (as svo_get_pose does), uploads the filter states and samples of its named slots in one copy, runs the filter of
 * all of them in ONE kernel launch (pose_filter.hip), downloads the states in one copy and stores them: every byte
 * of a slot's filter equals what the same svo_update_pose calls in the same order leave, for finite inputs (others:
 * the call terminates, the values are unspecified). The slot's pose, time stamp and trajectory are not touched.
 * SVO_POSE_SAMPLE_CHAIN: the sample measures the filtered pose of the slot's previous sample of this call, the
 * slot's first sample the slot's current pose (svo_get_pose; zeros on an empty slot): SlamApp::update_pose_from_imu
 * (src/app/slam_app.cpp:111-135) of one frame interval is one call without a round trip.
 * seqs, counts and samples are copied at submit time; filtered ([sum of counts][6], sample order, may be NULL) is
 * written by the groups' workers and valid after svo_wait.
 * A slot out of range or named twice, a negative count, an unknown flag bit, NULL samples with a positive total:
 * SVO_ERR_INVALID, nothing queued, the ctx stays usable. Device and pinned buffers are made by a group's first such
 * job (counted in svo_ctx_get_memory) and grow when a job needs more. */
int svo_submit_pose_updates(svo_ctx *ctx, const int *seqs, const int *counts, int n,
                            const svo_pose_sample *samples, float *filtered);
int svo_update_poses(svo_ctx *ctx, const int *seqs, const int *counts, int n,
                     const svo_pose_sample *samples, float *filtered);   /* submit + wait */
/* stage entry of the filter kernel: n_states filter states, every array in device memory, on the handle's stream.
 * state_in: per state statePost[12] | errorCovPost[144] (156 floats); state b runs samples [first[b], first[b + 1])
 * (first: n_states + 1 offsets, clamped to [0, n_samples)) in order, with A = I + dt, H = I, Q = 100 I of the
 * tracker's filter and R = diag(pose_var, speed_var); start_pose [n_states][6]: what a chained first sample measures.
 * state_out: per state statePre[12] | statePost[12] | errorCovPre[144] | errorCovPost[144] | gain[144] (456 floats)
 * after its last sample; filtered [n_samples][6] (may be NULL). A state without samples is neither read nor written,
 * and neither is anything outside the named ranges. samples: 8-byte aligned, the others 4-byte. */
int svo_pose_filter_batch(svo_handle *h, int n_states, const float *state_in, const float *start_pose,
                          const int *first, int n_samples, const svo_pose_sample *samples, float *state_out,
                          float *filtered);

/* ---- bulk export: the state of many slots in one ordered launch ------------
 * The reference reads its state one object at a time (get_frame / get_keyframes, src/lib/stereo_slam.cpp:273-289),
 * and so do the getters above: each waits for every queue of the ctx and makes twelve blocking copies per slot.
 * An export is the batched form: the groups that own a named slot pack the slots' keypoints into the getters'
 * records (svo_kp2d, svo_kp3d, svo_kp_info, byte for byte; svo_kp_info._pad is 0) with one kernel launch each and
 * deliver them into host or device memory; the host writes one svo_export_segment per named slot.
 *
 * Named slots: seqs == NULL names every slot in order (n is ignored); otherwise segment i describes slot seqs[i].
 * Placement: with R = svo_export_capacity's records per slot, group g packs its named slots densely, in named
 * order, from record (named slots of earlier groups) * R on; every segment's `first` is rounded up to a multiple
 * of 4, so a segment starts 16-byte aligned in all three arrays (given 16-byte aligned arrays; others work, more
 * slowly; 4-byte alignment is required). Records outside the segments are not written by the kernel: neither the
 * up to 3 records of padding between two segments nor the space between two groups. (Host mode copies a group's
 * used prefix, first segment to last, in one piece per array: there the padding records between the group's
 * segments receive unspecified bytes; the space after a group's last segment stays untouched.)
 * An empty slot (never started, or restarted) gives n = 0, frame_id = -1 and a zero pose. */
enum { SVO_EXPORT_FRAMES = 0,          /* the current frame of each named slot (what svo_get_frame_keypoints + svo_get_pose return) */
       SVO_EXPORT_LAST_KEYFRAMES = 1 };/* the newest keyframe of each named slot (svo_get_keyframe(seq, count-1)) */

typedef struct svo_export_segment {   /* 64 bytes, one per named slot, written by the host */
    int32_t seq, run;                 /* slot and ordinal of its run (svo_run_info.run)                    */
    int32_t frame_id;                 /* of the slot's current frame; -1: empty slot                        */
    int32_t keyframe_id;              /* LAST_KEYFRAMES: id exported (-1: the slot has none); FRAMES: -1   */
    int32_t is_keyframe;              /* svo_frame_stats.is_keyframe of the current frame                   */
    int32_t n;                        /* keypoints exported                                                 */
    int64_t first;                    /* they are records [first, first + n) of every array; multiple of 4 */
    float   pose[6];                  /* FRAMES: svo_get_pose; LAST_KEYFRAMES: the keyframe's pose          */
    float   time_stamp;               /* of the slot's current frame                                        */
    int32_t _pad;
} svo_export_segment;

typedef struct svo_export_dst {
    svo_export_segment *segments;     /* HOST memory always, >= n entries                                   */
    svo_kp2d *kps2d; svo_kp3d *kps3d; svo_kp_info *info;   /* host or device (mem); any may be NULL: skipped */
    int64_t capacity;                 /* records each non-NULL array holds                                  */
} svo_export_dst;

/* records one slot can take at most (the group's keypoint capacity: 2 * grid cells + 128, rounded up to a
 * multiple of 64), without a GPU. Settings svo_ctx_create rejects: SVO_ERR_INVALID */
int svo_export_capacity(const svo_camera_settings *cam, int width, int height, int *records_per_sequence);
/* Queued like a frame set: it sees every frame set and restart submitted before it and none submitted after it,
 * and it does not wait for other groups (only groups that own a named slot get work). dst (copied), the segments
 * and the arrays stay valid until svo_wait, after which everything is delivered. mem: SVO_MEM_HOST or
 * SVO_MEM_DEVICE, of the three arrays. Rejected with nothing queued: an index out of range or named twice, a bad
 * `what` or `mem`, a misaligned array (SVO_ERR_INVALID); dst->capacity < named slots * R while an array is given
 * (SVO_ERR_CAPACITY: the bound, not the counts, so that it can be checked here); a failed ctx, like
 * svo_submit_images. Host mode goes through a device staging block of (slots of the group) * R * 64 bytes per
 * group, made by the group's first host-mode export (svo_memory.device_bytes) and one copy per array; a ctx that
 * never exports pays nothing. An export that fails on the device side (a HIP error, e.g. no memory for the staging
 * block) is reported by svo_wait and fails the ctx like a frame that fails: what is still queued is dropped. */
int svo_submit_export(svo_ctx *ctx, int what, const int *seqs, int n, const svo_export_dst *dst, int mem);
int svo_export(svo_ctx *ctx, int what, const int *seqs, int n, const svo_export_dst *dst, int mem); /* submit + wait */
/* stage entry: n_sets SoA keypoint sets (host array of views onto device memory, sets[i].n valid entries;
 * every array 4-byte aligned) into AoS records at first[i] (host array, >= 0); kps2d / kps3d / info are device
 * memory, any may be NULL. The tracker's launch: keypoints [0, n) of a set are read, records [first, first + n)
 * written, nothing else. */
int svo_pack_keypoints(svo_handle *h, int n_sets, const svo_keypoints *sets, const int64_t *first,
                       svo_kp2d *kps2d, svo_kp3d *kps3d, svo_kp_info *info);

/* ---- map export: every keyframe of many slots as one compacted point cloud ------------
 * The reference's viewer protocol (`keyframes` / `get`, src/app/svo_slam_backend.cpp:18-110) sends EVERY keyframe of
 * the tracker: pose, kps3d and colours. svo_get_keyframe per id restates that with twelve blocking copies per
 * keyframe; svo_submit_export covers the newest keyframe only. A map export is the batched form for the whole map:
 * the groups that own a named slot write the keypoints of the slot's keyframes that pass a filter as 16-byte points,
 * densely, with map.hip's two kernels, and the host writes one svo_map_segment per named slot and one
 * svo_map_keyframe per exported keyframe.
 *
 * Filter: a keyframe copies the surviving points of earlier keyframes (merge_keypoints,
 * src/lib/depth_calculator.cpp:88-130), which keep their origin keyframe_id, while the depth filter writes refined
 * kps3d and flags back to the ORIGIN keyframe only (src/lib/stereo_slam.cpp:205-226): the copies in later keyframes
 * go stale. own_only keeps a point only in its origin keyframe, drop_flags / min_inliers select by quality. Only the
 * device holds these planes, so the compaction runs there.
 *
 * Order: a slot's kept points lie densely from region.first_point on: keyframes in ascending id, inside a keyframe
 * in ascending keypoint index. Stable: two runs give the same bytes.
 *
 * Polling: keyframes below svo_map_segment.keyframes_retired are no longer tracked, no write-back reaches them and
 * their points are final. A poller can pass from_keyframe = keyframes_retired of its last poll and keep what it has
 * of the keyframes below. Once that export is delivered it may trim them (svo_submit_trim_keyframes with below = the
 * from_keyframe it passed): they were final when the previous export ran, so the copies it holds are. The keyframes
 * in [from_keyframe, the newly reported keyframes_retired) become final in this export: it keeps those copies and
 * passes the new count next time. A trimmed slot exports from max(from_keyframe, first_keyframe) on. */
typedef struct svo_map_point {      /* 16 bytes */
    float   x, y, z;                /* kps3d, bits unchanged (world frame)                                  */
    uint8_t color[3];               /* r, g, b                                                              */
    uint8_t flags;                  /* SVO_IGNORE_* bits of the keypoint (other bits of its flags word: not kept) */
} svo_map_point;

typedef struct svo_map_filter {     /* all zero (or a NULL filter): every keypoint of every keyframe        */
    uint32_t drop_flags;            /* dropped if (flags & drop_flags) != 0; SVO_IGNORE_* bits only         */
    int32_t  own_only;              /* != 0: dropped if keyframe_id != id of the keyframe that holds it     */
    int32_t  min_inliers;           /* dropped if inlier_count < min_inliers (signed)                       */
    int32_t  _reserved;             /* 0, else SVO_ERR_INVALID                                              */
} svo_map_filter;

typedef struct svo_map_keyframe {   /* 48 bytes, host, one per exported keyframe                            */
    int32_t id, n_total, n, _pad;   /* its keypoints / those kept                                           */
    int64_t first;                  /* kept points are records [first, first + n) of `points`               */
    float   pose[6];
} svo_map_keyframe;

enum { SVO_MAP_COMPLETE = 0,
       SVO_MAP_TOO_SMALL = 1 };     /* a capacity of the slot's region was too small when the job ran: only its segment was written */

typedef struct svo_map_segment {    /* 64 bytes, host, one per named slot                                   */
    int32_t seq, run;               /* slot and ordinal of its run (svo_run_info.run)                       */
    int32_t frame_id;               /* of the slot's current frame; -1: empty slot (every count is 0)       */
    int32_t status;                 /* SVO_MAP_*                                                            */
    int32_t n_keyframes, keyframes_retired;   /* of the slot when the job ran                               */
    int32_t from_keyframe, n_exported;        /* keyframes [from_keyframe, from_keyframe + n_exported): from_keyframe =
                                                 max(the region's, first_keyframe); n_exported = max(0, n_keyframes -
                                                 from_keyframe) */
    int64_t n_points;               /* points kept (TOO_SMALL: 0)                                           */
    int64_t points_bound;           /* keypoints of the exported keyframes: the sum of their n_total        */
    float   time_stamp;             /* of the slot's current frame                                          */
    union {
        int32_t first_keyframe;     /* the slot's oldest resident keyframe (svo_keyframe_range.first; 0: untrimmed): */
        int32_t _pad[3];            /* _pad[0] of earlier versions; _pad[1], _pad[2]: 0                             */
    };
} svo_map_segment;

typedef struct svo_map_region {     /* where one named slot goes: the caller places every slot itself       */
    int64_t first_point;            /* its points are records [first_point, first_point + n_points) of dst->points */
    int64_t point_capacity;         /* records it may take: >= points_bound, or the slot comes back TOO_SMALL */
    int64_t first_keyframe_entry;   /* its keyframes are entries [first_keyframe_entry, + n_exported) of dst->keyframes */
    int32_t keyframe_capacity;      /* entries it may take: >= n_exported, or TOO_SMALL                     */
    int32_t from_keyframe;          /* >= 0; beyond the slot's count: nothing exported; below its first resident
                                       keyframe: from that one on                                            */
} svo_map_region;

typedef struct svo_map_dst {
    svo_map_segment  *segments;     /* HOST memory always, one per named slot                               */
    svo_map_keyframe *keyframes;    /* HOST memory always; NULL: every keyframe_capacity is 0               */
    svo_map_point    *points;       /* host or device (mem), 16-byte aligned; NULL: every point_capacity is 0 */
} svo_map_dst;

/* what an export of the slot from keyframe from_keyframe on (a trimmed slot: from its first resident keyframe, if that
 * is later) would need right now: *keyframes = n_exported,
 * *points_bound = the sum of their keypoint counts (either may be NULL). A getter: waits for the queues. */
int svo_map_size(svo_ctx *ctx, int seq, int from_keyframe, int *keyframes, int64_t *points_bound);
/* Queued exactly as svo_submit_export is (seqs == NULL names every slot in order, n is ignored; segment i and
 * regions[i] belong to slot seqs[i]): it sees every frame set, restart, load and pose update submitted before it and
 * none submitted after; only the groups that own a named slot get work and no group waits for another; the slot is
 * not changed (its deferred pose-filter update is flushed first). regions, filter and dst are copied; segments,
 * keyframes and points stay valid until svo_wait, after which everything is delivered. Regions must not overlap.
 * Sizes: keyframe counts grow while frames are queued, so they are only known when the job runs. A slot with
 * n_exported > keyframe_capacity or points_bound > point_capacity gets status SVO_MAP_TOO_SMALL: its segment carries
 * the counts needed, nothing else of the slot is written, the other slots are delivered, the ctx does not fail and
 * svo_wait returns SVO_OK (the rule of snapshots). The check is on the bound, never on the kept count, so it is made
 * before any launch and the kernels cannot overrun a region. Of a region exactly records [first_point, first_point
 * + n_points) and entries [first_keyframe_entry, + n_exported) are written.
 * Rejected with SVO_ERR_INVALID and nothing queued: a slot out of range or named twice, a bad mem (SVO_MEM_HOST or
 * SVO_MEM_DEVICE, of `points`), NULL segments, NULL keyframes or points together with a positive capacity, a
 * negative region field, a misaligned points, drop_flags bits that are no SVO_IGNORE_* bit, _reserved != 0; a
 * failed ctx, as in svo_submit_images.
 * Every group keeps a small block of counts (per keyframe and tile of a job) and, in host mode, a staging block of
 * points: made by the group's first (host-mode) map export, grown when outgrown, counted in svo_ctx_get_memory. Host
 * mode copies each named slot's kept prefix out in one piece; the per-keyframe kept counts come back in one copy per
 * group. A ctx that never exports a map allocates, launches and copies nothing more. */
int svo_submit_export_map(svo_ctx *ctx, const int *seqs, int n, const svo_map_region *regions,
                          const svo_map_filter *filter, const svo_map_dst *dst, int mem);
int svo_export_map(svo_ctx *ctx, const int *seqs, int n, const svo_map_region *regions,
                   const svo_map_filter *filter, const svo_map_dst *dst, int mem);   /* submit + wait */
/* stage entry of the two kernels: region r holds the SoA sets [set_begin[r], set_begin[r + 1]) (set_begin: host,
 * n_regions + 1 entries from 0 on, ascending; sets: host array of views onto device memory, of which kps3d, flags,
 * keyframe_id, inlier_count and color are read: 4-byte aligned); own_id[s] (host): the keyframe id set s is held
 * by; first[r] (host, >= 0): the record region r starts at. The kept points of a region leave densely from
 * points[first[r]] on, in set order and keypoint order (points: device, 16-byte aligned, or NULL: only counts);
 * counts[s] (device, one per set, or NULL) receives the points kept of set s. The tracker's launches (chunked when
 * the diagnostic SVO_MAP_TABLE_TILES bounds the tile table): keypoints [0, n) of the five planes of a set are read,
 * records [first[r], + kept of r) and every counts[s] written, nothing else. Complete on return. */
int svo_pack_map_points(svo_handle *h, int n_regions, const int32_t *set_begin, const svo_keypoints *sets,
                        const int32_t *own_id, const int64_t *first, const svo_map_filter *filter,
                        svo_map_point *points, int32_t *counts);

/* ---- views: the images of frames and newest keyframes of many slots in one queued job ------------
 * The reference hands images to its caller: Frame and KeyFrame carry stereo_image (src/include/stereo_slam_types.hpp:120),
 * and its consumers read frame.stereo_image.left[0]: the test app's window (draw_frame, src/app/main.cpp:40-118: the
 * last keyframe and the current frame, a marker per keypoint) and the AR demo's video surface
 * (src/ar-app/opencvimageprovider.cpp:33,59). Here the gray images are made on the device (input formats,
 * rectification, pyramids) and only a snapshot moved them out. A view job is the batched reader: the groups that own a
 * named slot render one image per slot with one kernel launch each (view.hip) and deliver it into host or device
 * memory; the host writes one svo_view_segment per named slot. Two forms: the plain gray plane, or gray expanded to
 * RGB with one marker per keypoint, composed on the device, where keypoints, colours and flags live.
 *
 * Layout: rows are dense, pitch = cols * bytes per pixel; image_bytes = rows * pitch rounded up to a multiple of 256;
 * named slot i of a job goes to offset = i * image_bytes of dst->pixels, whatever group owns it. Of a slot exactly
 * rows * pitch bytes from its offset on are written; a slot whose status is SVO_VIEW_NONE writes only its segment.
 *
 * Markers: the project's own statement of cv::drawMarker(img, p, color, type, size) at thickness 1 as draw_frame
 * calls it, for the two marker types the app uses; both are axis-aligned runs of pixels. Not restated: the text
 * overlay (putText) and the x2 cv::resize of the app's window.
 *   centre  c = (trunc(x * 2^-level), trunc(y * 2^-level)), truncated toward zero (Point(float, float)); a keypoint
 *           whose scaled coordinate is not finite or has magnitude >= 2^15 draws nothing
 *   size    s = size_temporary if the keypoint has SVO_IGNORE_TEMPORARY, else size (the app: 10 / 20 for a frame, 10
 *           for a keyframe)
 *   cross   type SVO_KP_FAST: the pixels (cx - s/2 .. cx + s/2, cy) and (cx, cy - s/2 .. cy + s/2); integer
 *           division, ends inclusive
 *   square  any other type: with s' = (int)(s * 0.8), the border of [cx - s'/2, cx + s'/2] x [cy - s'/2, cy + s'/2]
 *   colour  bytes r, g, b of the keypoint's colour into channels 0, 1, 2 (the app draws Scalar(r, g, b) into a
 *           GRAY2RGB image); every other pixel is (g, g, g); the fourth byte of RGBA is 255
 *   order   keypoints are drawn in ascending index and a later one overwrites: a pixel takes the colour of the
 *           highest-index keypoint that is not dropped and whose marker covers it
 *   pixels outside the image are dropped. */
enum { SVO_PLANE_LEFT = 0, SVO_PLANE_RIGHT = 1 };
enum { SVO_PIXEL_GRAY8 = 0, SVO_PIXEL_RGB8 = 1, SVO_PIXEL_RGBA8 = 2 };   /* 1, 3, 4 bytes per pixel; A = 255 */
enum { SVO_VIEW_OK = 0,
       SVO_VIEW_NONE = 1 };         /* an empty slot, no keyframe yet, or the keyframe has given its image set back */

typedef struct svo_view_style {     /* what one job draws; copied at submit                                 */
    int32_t  plane;                 /* SVO_PLANE_*                                                          */
    int32_t  level;                 /* LEFT: pyramid level 0 .. max_pyramid_levels - 1 ((width >> level) x (height >> level));
                                       RIGHT: 0                                                             */
    int32_t  pixel;                 /* SVO_PIXEL_*                                                          */
    int32_t  markers;               /* 0: the plane only; 1: and one marker per keypoint (LEFT and RGB8 / RGBA8 only) */
    uint32_t drop_flags;            /* keypoints with (flags & drop_flags) != 0 get no marker; SVO_IGNORE_* bits only */
    int32_t  size, size_temporary;  /* marker size without / with SVO_IGNORE_TEMPORARY, 0 .. 64             */
    int32_t  _reserved;             /* 0                                                                    */
} svo_view_style;

typedef struct svo_view_segment {   /* 64 bytes, host, one per named slot                                   */
    int32_t seq, run;               /* slot and ordinal of its run (svo_run_info.run)                       */
    int32_t frame_id;               /* of the slot's current frame; -1: empty slot                          */
    int32_t keyframe_id;            /* LAST_KEYFRAMES: the keyframe shown (-1: the slot has none); FRAMES: -1 */
    int32_t status;                 /* SVO_VIEW_*                                                           */
    int32_t n;                      /* keypoints of the set the markers come from                           */
    int64_t offset;                 /* the image is bytes [offset, offset + rows * pitch) of dst->pixels    */
    float   pose[6];                /* FRAMES: svo_get_pose; LAST_KEYFRAMES: the keyframe's pose            */
    float   time_stamp;             /* of the slot's current frame                                          */
    int32_t _pad;
} svo_view_segment;

typedef struct svo_view_dst {
    svo_view_segment *segments;     /* HOST memory always, >= n entries                                     */
    uint8_t *pixels;                /* host or device (mem); 4-byte aligned (16-byte aligned: the wide stores) */
    int64_t capacity;               /* bytes `pixels` holds                                                 */
} svo_view_dst;

/* the shape of one image of a job with that style in a ctx of these settings, without a GPU (any out pointer may be
 * NULL). Settings svo_ctx_create rejects, or a style a job rejects: SVO_ERR_INVALID */
int svo_view_size(const svo_camera_settings *cam, int width, int height, const svo_view_style *style,
                  int *cols, int *rows, int64_t *pitch, int64_t *image_bytes);
/* what: SVO_EXPORT_FRAMES (the image set of the slot's current frame; a slot that sat steps out shows its last frame;
 * under SVO_MEM_DEVICE_BORROW level 0 and the right image are the caller's buffers, which the validity rule above
 * keeps alive) or SVO_EXPORT_LAST_KEYFRAMES (the image set and keypoints of the newest keyframe; once it has given its
 * images back the status is SVO_VIEW_NONE). Queued exactly as svo_submit_export is (seqs == NULL names every slot in
 * order, n is ignored): the job sees every frame set, restart, load and pose update submitted before it and none
 * submitted after, only groups that own a named slot get work, no group waits for another, the slot is not changed
 * (its deferred pose-filter update is flushed first). style and dst are copied; segments and pixels stay valid until
 * svo_wait, after which everything is delivered. mem: SVO_MEM_HOST or SVO_MEM_DEVICE, of `pixels`.
 * Rejected with SVO_ERR_INVALID and nothing queued: a slot out of range or named twice; a bad what, mem, plane, level,
 * pixel or size; markers with RIGHT or with GRAY8; drop_flags bits that are no SVO_IGNORE_* bit; _reserved != 0; NULL
 * segments; pixels NULL or not 4-byte aligned; a failed ctx, as in svo_submit_images. SVO_ERR_CAPACITY: dst->capacity
 * < named slots * image_bytes (the bound, so it is checked here).
 * Host mode: a group renders its named slots densely into a device staging block, made by the group's first host-mode
 * view job and replaced when outgrown (svo_memory.device_bytes), and copies each run of consecutive named slots out
 * in one piece. Device mode writes in place and allocates nothing. A ctx that never asks for a view allocates,
 * launches and copies nothing more. */
int svo_submit_export_views(svo_ctx *ctx, int what, const int *seqs, int n, const svo_view_style *style,
                            const svo_view_dst *dst, int mem);
int svo_export_views(svo_ctx *ctx, int what, const int *seqs, int n, const svo_view_style *style,
                     const svo_view_dst *dst, int mem);   /* submit + wait */
/* stage entry of the kernel: n images in the tracker's launch (chunked when the diagnostic SVO_VIEW_TABLE_TILES bounds
 * the tile table). src[i].image: the gray plane (device memory, any base address, stride >= width; its width x height
 * is the output's cols x rows); src[i].kps: the set the markers come from, of which kps2d, flags, level_type and color
 * are read (device, 4-byte aligned; ignored without style->markers). Image i goes to pixels + offset[i] (host array,
 * >= 0, multiples of 4; pixels: device, 4-byte aligned), rows dense. style->plane is not used and style->level (0 ..
 * SVO_MAX_PYRAMID_LEVELS - 1) only scales the keypoints. Exactly the images' bytes are written. Complete on return. */
typedef struct svo_view_src {
    svo_image     image;
    svo_keypoints kps;
} svo_view_src;
int svo_render_views(svo_handle *h, int n, const svo_view_src *src, const int64_t *offset,
                     const svo_view_style *style, uint8_t *pixels);

/* ---- scene: the viewer's 3-D picture of the maps of many slots in one queued job ------------
 * The reference's second window is its 3-D viewer (src/qt-viewer/PointCloudViewer.qml, src/python/pointcloudviewer.py):
 * every keyframe's points as depth-tested squares of fixed size on white, the trajectory as a red line strip, a blue
 * wire frustum per keyframe and a green one at the current pose, seen through a perspective camera with front / top /
 * side presets. A scene job is that picture for many slots: the groups that own a named slot render one image per
 * slot with one kernel launch each (scene.hip) from the keyframe planes on the device and from line records the host
 * builds from the trajectory and the poses, and deliver it into host or device memory; the host writes one
 * svo_scene_segment per named slot.
 *
 * The picture is the project's own statement of the viewer's scene, not GL's rasteriser (which is not specified to
 * the bit). All arithmetic is float32 in the order written, without contraction; integer parts are exact.
 *   camera   svo_scene_camera: V = view[12], the rows of a 3x4 world -> camera matrix (camera frame as the tracker's:
 *            x right, y down, z forward), and f, cx, cy, near
 *   T(x,y,z) c_k = ((V[4k] * x + V[4k+1] * y) + V[4k+2] * z) + V[4k+3],  k = 0, 1, 2
 *   point    (class 3) dropped unless every c_k is finite and c_2 >= near.  u = (f * c_0) / c_2 + cx,
 *            v = (f * c_1) / c_2 + cy; dropped unless |u| < 2^15 and |v| < 2^15.  px = floor(u), py = floor(v); it
 *            covers the s x s pixels [px - (s-1)/2, px - (s-1)/2 + s - 1] x [py - (s-1)/2, py - (s-1)/2 + s - 1]
 *            (integer division), s = point_size; its depth is c_2, its colour the keypoint's r, g, b (the QML swaps r
 *            and b; that quirk is not restated)
 *   line     A -> B (classes 0 .. 2), a = T(A), b = T(B): dropped if any coordinate is not finite or both a_2 and
 *            b_2 < near. If exactly one end, say a, has a_2 < near: t = (near - a_2) / (b_2 - a_2),
 *            a_k := a_k + t * (b_k - a_k) for k = 0, 1, a_2 := near (the same with the roles swapped when b is the
 *            near end); dropped if the result is not finite. Both ends are projected as a point is; the line is
 *            dropped if either end fails the 2^15 rule. X = floor(u), Y = floor(v), dx = X1 - X0, dy = Y1 - Y0,
 *            n = max(|dx|, |dy|). Pixel i = 0 .. n is (X0 + rdiv(i * dx, n), Y0 + rdiv(i * dy, n)) with
 *            rdiv(p, n) = floor((2 p + n) / (2 n)) in int64; n = 0: the single pixel (X0, Y0). Its depth is
 *            z_i = z0 + (z1 - z0) * ((float)i / (float)n), z0 for n = 0: linear on the screen, NOT
 *            perspective-correct. One pixel wide.
 *   pixel    every element that covers it offers the 64-bit key  bits(depth) << 32 | cls << 24 | r << 16 | g << 8 | b;
 *            the pixel shows r, g, b of the SMALLEST key: the nearest element wins; at equal depth a line beats a
 *            point and the current-pose frustum beats everything; inside a class the smaller colour word wins. The
 *            result depends on no drawing order and two runs give the same bytes. A pixel nobody covers shows
 *            `background`; the fourth byte of RGBA is 255. Pixels outside the image are dropped.
 * Elements of a slot, each drawn only if its bit of style.show is set:
 *   POINTS      the keypoints of keyframes from_keyframe .. that pass style.filter (a svo_map_filter, with exactly
 *               the meaning map export gives it)
 *   TRAJECTORY  class 2, trajectory_rgb: the lines between consecutive positions of svo_get_trajectory;
 *               trajectory_tail = k > 0 draws the newest k poses only (k - 1 lines)
 *   KEYFRAMES   class 1, keyframe_rgb: a frustum per keyframe from from_keyframe on
 *   POSE        class 0, pose_rgb: a frustum at svo_get_pose
 * Frustum of a pose (t, r): camera-frame vertices 0, (-w, h, d), (-w, -h, d), (w, -h, d), (w, h, d); the 8 edges of
 * the QML's index buffer (0-1, 0-2, 0-3, 0-4, 1-2, 2-3, 3-4, 4-1); w, h, d from the style (the viewer: 0.1, 0.08,
 * 0.07). World vertex: ((R[3k] * vx + R[3k+1] * vy) + R[3k+2] * vz) + t_k, R the float `rot` of
 * PoseManager::set_pose (Rodrigues in double with the sin / cos of svo_libm.h, rounded to float). The QML orients
 * its frusta with fromEulerAngles; the tracker's Rodrigues is used instead.
 * Layout, as for the views: rows are dense, pitch = cols * bytes per pixel; image_bytes = rows * pitch rounded up to
 * a multiple of 256; named slot i of a job goes to offset = i * image_bytes of dst->pixels; of a slot exactly
 * rows * pitch bytes are written; a slot whose status is SVO_SCENE_NONE writes only its segment.
 * Not drawn: text, anti-aliasing, line widths; there is no orbit controller and no fitting of the camera to a map. */
enum { SVO_SCENE_POINTS = 1, SVO_SCENE_TRAJECTORY = 2, SVO_SCENE_KEYFRAMES = 4, SVO_SCENE_POSE = 8 };   /* style.show */
enum { SVO_SCENE_CLASS_POSE = 0, SVO_SCENE_CLASS_KEYFRAME = 1, SVO_SCENE_CLASS_TRAJECTORY = 2, SVO_SCENE_CLASS_POINT = 3 };
enum { SVO_SCENE_OK = 0,
       SVO_SCENE_NONE = 1 };          /* an empty slot */

typedef struct svo_scene_camera {     /* 64 bytes */
    float view[12];                   /* rows of the 3x4 world -> camera matrix                              */
    float f, cx, cy;                  /* focal length and principal point, pixels                            */
    float near;                       /* elements nearer than this are dropped / clipped                     */
} svo_scene_camera;                   /* rejected: an entry that is not finite, f <= 0, near <= 0            */

typedef struct svo_scene_style {      /* what one job draws; copied at submit                                */
    int32_t  cols, rows;              /* of every image: 1 .. 4096                                           */
    int32_t  pixel;                   /* SVO_PIXEL_RGB8 or SVO_PIXEL_RGBA8                                   */
    int32_t  point_size;              /* 1 .. 16                                                             */
    uint32_t background, trajectory_rgb, keyframe_rgb, pose_rgb;   /* r << 16 | g << 8 | b; the top byte 0   */
    float    frustum_w, frustum_h, frustum_d;   /* finite                                                   */
    uint32_t show;                    /* SVO_SCENE_* bits                                                    */
    int32_t  from_keyframe;           /* >= 0: points and frusta of the resident keyframes from this one on  */
    int32_t  trajectory_tail;         /* 0: the whole trajectory; k > 0: its newest k poses                  */
    svo_map_filter filter;            /* which keypoints are points                                          */
    int32_t  _reserved;               /* 0                                                                   */
} svo_scene_style;

typedef struct svo_scene_line {       /* 32 bytes: one line of the stage entry                               */
    float    a[3], b[3];              /* world                                                               */
    uint32_t cls_rgb;                 /* cls << 24 | r << 16 | g << 8 | b, cls 0 .. 2                        */
    uint32_t _pad;                    /* 0                                                                   */
} svo_scene_line;

typedef struct svo_scene_segment {    /* 64 bytes, host, one per named slot                                  */
    int32_t  seq, run;                /* slot and ordinal of its run (svo_run_info.run)                      */
    int32_t  frame_id;                /* of the slot's current frame; -1: empty slot                         */
    uint16_t status;                  /* SVO_SCENE_*                                                         */
    uint16_t n_keyframes;             /* of the slot when the job ran, its low 16 bits (ids outlive a trimmed table)  */
    int32_t  from_keyframe;           /* the style's                                                         */
    int32_t  n_keypoints;             /* keypoints considered: those of keyframes from_keyframe .. (0 without POINTS) */
    int32_t  n_poses;                 /* trajectory poses drawn (0 without TRAJECTORY)                       */
    float    time_stamp;              /* of the slot's current frame                                         */
    int64_t  offset;                  /* the image is bytes [offset, offset + rows * pitch) of dst->pixels   */
    float    pose[6];                 /* svo_get_pose                                                        */
} svo_scene_segment;

typedef struct svo_scene_dst {
    svo_scene_segment *segments;      /* HOST memory always, >= n entries                                    */
    uint8_t *pixels;                  /* host or device (mem); 4-byte aligned (16-byte aligned: the wide stores) */
    int64_t capacity;                 /* bytes `pixels` holds                                                */
} svo_scene_dst;

/* pitch and image_bytes of one image of a job with that style, without a GPU (either may be NULL). A style a job
 * rejects: SVO_ERR_INVALID */
int svo_scene_size(const svo_scene_style *style, int64_t *pitch, int64_t *image_bytes);
/* a camera at `eye` looking at `centre`, without a GPU: z_c = normalize(centre - eye), x_c = normalize(cross(-up,
 * z_c)), y_c = cross(z_c, x_c); row k of view = (axis_k, -axis_k . eye); f = (rows / 2) / tan(fov_y / 2), cx =
 * cols / 2, cy = rows / 2; computed in double, stored as float. The viewer's presets (fov 45, near 0.1): front eye
 * (0, 0, -1) up (0, -1, 0), top eye (0, -5, 0) up (0, 0, 1), side eye (-5, 0, 0) up (0, -1, 0), centre 0.
 * SVO_ERR_INVALID: an argument that is not finite, eye == centre, up parallel to the viewing direction, fov_y not
 * within (0, 180), cols or rows < 1, near <= 0, or a result a job rejects. */
int svo_scene_look_at(const float eye[3], const float centre[3], const float up[3], float fov_y_deg, int cols, int rows,
                      float near, svo_scene_camera *camera);
/* the 8 world lines (a, b) of the frustum of `pose` with dims = (w, h, d), in the order of the index buffer, without
 * a GPU */
int svo_scene_frustum(const float pose[6], const float dims[3], float out[8][6]);
/* Queued exactly as svo_submit_export_views is (seqs == NULL names every slot in order, n is ignored): the job sees
 * every frame set, restart, load and pose update submitted before it and none submitted after, only groups that own a
 * named slot get work, no group waits for another, the slot is not changed (its deferred pose-filter update is
 * flushed first). cameras: ONE PER NAMED SLOT, cameras[i] belongs to seqs[i] (pass the same camera n times for one
 * view of all). style, cameras and dst are copied; segments and pixels stay valid until svo_wait, after which
 * everything is delivered. mem: SVO_MEM_HOST or SVO_MEM_DEVICE, of `pixels`.
 * Rejected with SVO_ERR_INVALID and nothing queued: a slot out of range or named twice; a bad mem; a style or a
 * camera out of the ranges above (GRAY8, unknown show bits, a colour with a top byte, filter bits that are no
 * SVO_IGNORE_* bit, _reserved != 0, ...); NULL cameras or segments; pixels NULL or not 4-byte aligned; a failed ctx,
 * as in svo_submit_images. SVO_ERR_CAPACITY: dst->capacity < named slots * image_bytes.
 * The host builds the trajectory and frustum lines of the group's named slots (svo_scene_frustum) and uploads them
 * with the table of keyframe sets in one copy per group, into an input block made by the group's first scene job and
 * replaced when outgrown. Host mode: a group renders its named slots densely into a device staging block (likewise)
 * and copies each run of consecutive named slots out in one piece. Device mode writes in place. Both blocks count in
 * svo_ctx_get_memory (svo_memory.device_bytes). A ctx that never asks for a scene allocates, launches and copies
 * nothing more. */
int svo_submit_export_scenes(svo_ctx *ctx, const int *seqs, int n, const svo_scene_style *style,
                             const svo_scene_camera *cameras, const svo_scene_dst *dst, int mem);
int svo_export_scenes(svo_ctx *ctx, const int *seqs, int n, const svo_scene_style *style,
                      const svo_scene_camera *cameras, const svo_scene_dst *dst, int mem);   /* submit + wait */
/* stage entry of the kernel: n images in the tracker's launch (chunked when the diagnostic SVO_SCENE_TABLE_TILES
 * bounds the tile table). Image i is src[i].cols x src[i].rows (1 .. 4096 each; style->cols and rows are not used)
 * and shows, through cameras[i], the n_sets SoA keyframe sets src[i].sets (host array of views onto device memory, of
 * which kps3d, flags, keyframe_id, inlier_count and color are read: 4-byte aligned; own_id[s], host: the keyframe id
 * set s is held by, as svo_pack_map_points takes them) filtered by style->filter as points of style->point_size, and
 * the n_lines lines src[i].lines (device memory, 16-byte aligned). style->show, from_keyframe, trajectory_tail, the
 * three line colours and the frustum are not used. Image i goes to pixels + offset[i] (host array, >= 0, multiples
 * of 4; pixels: device, 4-byte aligned), rows dense. Exactly the images' bytes are written. Complete on return. */
typedef struct svo_scene_src {
    int32_t cols, rows;
    int32_t n_sets, n_lines;
    const svo_keypoints *sets;
    const int32_t *own_id;
    const svo_scene_line *lines;
} svo_scene_src;
int svo_render_scene(svo_handle *h, int n, const svo_scene_src *src, const svo_scene_camera *cameras,
                     const int64_t *offset, const svo_scene_style *style, uint8_t *pixels);

/* ---- ar: lit meshes over the camera image of many slots in one queued job ------------
 * The reference's third program is its AR demo (src/ar-app/): the left image of the current frame as the video
 * surface (opencvimageprovider.cpp:33,59), a camera at the tracked pose (slam.cpp:19-40, AnimatedEntity.qml:12-36)
 * whose frustum comes from the pinhole intrinsics (AnimatedEntity.qml:15-22), and an entity fixed in the world
 * (AnimatedEntity.qml:51-59, ObjectEntity.qml: a mesh and a directional light). An ar job is that picture for many
 * slots: the groups that own a named slot draw the job's mesh instances, flat shaded and depth tested, over the left
 * level-0 plane of each slot's current frame with two kernel launches each (ar.hip) and deliver one image per slot
 * into host or device memory; the host writes one svo_ar_segment per named slot.
 *
 * The picture is the project's own statement, not GL's rasteriser. All arithmetic is float32 in the order written,
 * without contraction; integer parts are exact (int64 where said).
 *   output     one image per named slot, W x H of the ctx (level 0), SVO_PIXEL_RGB8 or SVO_PIXEL_RGBA8. Layout as for
 *              views and scenes: rows dense, pitch = W * bytes per pixel; image_bytes = H * pitch rounded up to a
 *              multiple of 256; named slot i of a job at offset = i * image_bytes of dst->pixels; of a slot exactly
 *              H * pitch bytes are written; the fourth byte of RGBA is 255; a slot whose status is SVO_AR_NONE writes
 *              only its segment
 *   background the left level-0 plane of the slot's current frame: the plane a view job with what = FRAMES, plane =
 *              LEFT, level = 0 shows (under SVO_MEM_DEVICE_BORROW the caller's buffer, as for views). A pixel no
 *              triangle covers shows (g, g, g)
 *   camera     svo_ar_camera: V = view[12], the rows of the 3x4 world -> camera matrix, and fx, fy, cx, cy. Of a slot
 *              (svo_ar_camera_of_pose): with (t, r) = svo_get_pose and R the float `rot` of PoseManager::set_pose
 *              (Rodrigues in double with the sin / cos of svo_libm.h, rounded to float: the R of the scene's frusta),
 *              view[4k + j] = R[3j + k] (row k of R transposed) and
 *              view[4k + 3] = -(((R[k] * t_0) + (R[3 + k] * t_1)) + (R[6 + k] * t_2)); this is the mapping of
 *              project_keypoints (src/lib/transform_keypoints.cpp:23-45: subtract the translation, rotate by -r) up
 *              to float rounding; fx, fy, cx, cy are the intrinsics of the slot's rig. The distortion coefficients
 *              are NOT applied (the tracked plane is rectified): straight edges stay straight
 *   vertex     (x, y, z) of instance M = model[12]: world w_k = ((M[4k] * x + M[4k+1] * y) + M[4k+2] * z) + M[4k+3];
 *              camera c_k = ((V[4k] * w_0 + V[4k+1] * w_1) + V[4k+2] * w_2) + V[4k+3] (the scene's T);
 *              u = (fx * c_0) / c_2 + cx, v = (fy * c_1) / c_2 + cy
 *   triangle   vertices 0, 1, 2 of a mesh triangle. Dropped when a vertex index is outside [0, n_vertices) (the job
 *              rejects such a mesh at submit; the stage entry cannot read device memory on the host), when any w_k or
 *              c_k of a vertex is not finite, when any vertex has c_2 < near (NO clipping against the near plane:
 *              tessellate objects that come close), or when any |u| or |v| is not < 2^15. Otherwise
 *              X = (int)floorf(u * 16), Y = (int)floorf(v * 16): 4 sub-pixel bits, |X|, |Y| < 2^19
 *   coverage   in int64 at the pixel centre P = (16 px + 8, 16 py + 8):
 *              E_0 = (X2 - X1)(Py - Y1) - (Y2 - Y1)(Px - X1), E_1 the same for the edge 2 -> 0, E_2 for 0 -> 1;
 *              A = E_0 + E_1 + E_2 = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0), twice the area, the same at every
 *              pixel. A == 0: dropped. A < 0: E_0, E_1, E_2 and A are negated (both faces are drawn). The pixel is
 *              covered iff every E_k >= 0: inclusive, so two triangles that share an edge leave no hole; the key
 *              settles the pixels both cover
 *   depth      l_k = (float)E_k / (float)A (int64 -> float, round to nearest even); z = (l_0 * c2_0 + l_1 * c2_1) +
 *              l_2 * c2_2 with c2_k the c_2 of vertex k: linear on the screen like the scene's lines, NOT
 *              perspective-correct. z > 0, so its bits order as the values do
 *   colour     flat per triangle, in world space: e1 = w1 - w0, e2 = w2 - w0,
 *              n = (e1_y * e2_z - e1_z * e2_y, e1_z * e2_x - e1_x * e2_z, e1_x * e2_y - e1_y * e2_x),
 *              q = (n_x * n_x + n_y * n_y) + n_z * n_z, d = (n_x * L_x + n_y * L_y) + n_z * L_z with L = style.light,
 *              t = fabsf(d) / sqrtf(q); s = 0 when q == 0 or t is a NaN, else t when t < 1, else 1;
 *              shade = ambient + (1 - ambient) * s; channel c' = min(255, (int)(c * shade + 0.5f)) for c = r, g, b
 *              of the mesh's per-triangle rgb if it has one, else of the instance's rgb. L is used as given (not
 *              normalised): a unit vector gives Lambert's |cos|
 *   pixel      every covering triangle offers the 64-bit key  bits(z) << 32 | r' << 16 | g' << 8 | b'; the pixel
 *              shows r', g', b' of the SMALLEST key. No drawing order enters: two runs give the same bytes.
 * Not drawn: near clipping, textures, smooth shading, spot lights, transparency, anti-aliasing, lens distortion, the
 * scene's points and frusta. */
enum { SVO_AR_OK = 0,
       SVO_AR_NONE = 1 };             /* an empty slot */
enum { SVO_AR_MAX_TRIANGLES = 65536 };   /* instanced triangles of one image (slot) at most */

typedef struct svo_ar_camera {        /* 64 bytes */
    float view[12];                   /* rows of the 3x4 world -> camera matrix                              */
    float fx, fy, cx, cy;             /* pinhole intrinsics, pixels                                          */
} svo_ar_camera;                      /* rejected: an entry that is not finite, fx <= 0 or fy <= 0           */

typedef struct svo_ar_mesh {          /* 40 bytes; HOST memory, copied at submit                             */
    const float   *vertices;          /* n_vertices x (x, y, z)                                              */
    const int32_t *triangles;         /* n_triangles x 3 vertex indices, each 0 .. n_vertices - 1            */
    const uint32_t *rgb;              /* n_triangles colours r << 16 | g << 8 | b, or NULL: the instance's   */
    int32_t n_vertices, n_triangles;  /* >= 0                                                                */
    int64_t _reserved;                /* 0                                                                   */
} svo_ar_mesh;

typedef struct svo_ar_instance {      /* 64 bytes */
    float    model[12];               /* rows of the 3x4 mesh -> world matrix, finite                        */
    int32_t  mesh;                    /* index into the job's meshes                                         */
    uint32_t rgb;                     /* r << 16 | g << 8 | b; the top byte 0                                */
    int32_t  _reserved[2];            /* 0                                                                   */
} svo_ar_instance;

typedef struct svo_ar_style {         /* 32 bytes; what one job draws; copied at submit                      */
    int32_t pixel;                    /* SVO_PIXEL_RGB8 or SVO_PIXEL_RGBA8                                   */
    float   light[3];                 /* L, world, finite (the demo: 0, 0, 1)                                */
    float   ambient;                  /* 0 .. 1                                                              */
    float   near;                     /* > 0, finite (the demo: 0.01)                                        */
    int32_t _reserved[2];             /* 0                                                                   */
} svo_ar_style;

typedef struct svo_ar_segment {       /* 64 bytes, host, one per named slot                                  */
    int32_t  seq, run;                /* slot and ordinal of its run (svo_run_info.run)                      */
    int32_t  frame_id;                /* of the slot's current frame; -1: empty slot                         */
    uint16_t status;                  /* SVO_AR_*                                                            */
    uint16_t _pad;
    int32_t  n_instances;             /* instances the slot shows                                            */
    int32_t  n_triangles;             /* triangles offered: the sum of their meshes' (0 with SVO_AR_NONE)    */
    float    time_stamp;              /* of the slot's current frame                                         */
    int32_t  _pad2;
    int64_t  offset;                  /* the image is bytes [offset, offset + H * pitch) of dst->pixels      */
    float    pose[6];                 /* svo_get_pose                                                        */
} svo_ar_segment;

typedef struct svo_ar_dst {
    svo_ar_segment *segments;         /* HOST memory always, >= n entries                                    */
    uint8_t *pixels;                  /* host or device (mem); 4-byte aligned (16-byte aligned: the wide stores) */
    int64_t capacity;                 /* bytes `pixels` holds                                                */
} svo_ar_dst;

/* pitch and image_bytes of one image of a job with that style in a ctx of these settings, without a GPU (either may
 * be NULL). Settings svo_ctx_create rejects, or a style a job rejects: SVO_ERR_INVALID */
int svo_ar_size(const svo_camera_settings *cam, int width, int height, const svo_ar_style *style, int64_t *pitch,
                int64_t *image_bytes);
/* the camera of a slot at `pose` (t, r) with the intrinsics of `cam`, as stated above, without a GPU */
int svo_ar_camera_of_pose(const float pose[6], const svo_camera_settings *cam, svo_ar_camera *camera);
/* Queued exactly as svo_submit_export_scenes is (seqs == NULL names every slot in order, n is ignored): the job sees
 * every frame set, restart, load and pose update submitted before it and none submitted after, only groups that own a
 * named slot get work, no group waits for another, the slot is not changed (its deferred pose-filter update is
 * flushed first). first == NULL: every named slot shows instances [0, n_instances) (the demo: one object, seen by
 * all); else first[n + 1] (seqs == NULL: n = the ctx's slots) gives named slot i the instances [first[i],
 * first[i + 1]). style, meshes (with everything they point to), instances and first are copied at submit; segments
 * and pixels stay valid until svo_wait, after which everything is delivered. mem: SVO_MEM_HOST or SVO_MEM_DEVICE, of
 * `pixels`.
 * Rejected with SVO_ERR_INVALID and nothing queued: a slot out of range or named twice; a bad mem or pixel (GRAY8);
 * a light, ambient, near or model entry that is not finite; ambient outside 0 .. 1; near <= 0; an instance colour or
 * a mesh colour with a top byte; an instance's mesh outside [0, n_meshes); a vertex index outside [0, n_vertices); a
 * negative count; a `first` that starts below 0, does not ascend or does not end at n_instances; NULL where
 * data is needed (segments, pixels, meshes with n_meshes > 0, instances with n_instances > 0, the arrays of a mesh
 * with a positive count); pixels not 4-byte aligned; _reserved != 0; a failed ctx, as in svo_submit_images.
 * SVO_ERR_CAPACITY: dst->capacity < named slots * image_bytes, or a slot with more than SVO_AR_MAX_TRIANGLES
 * instanced triangles.
 * Per job and group one pinned input block (meshes, instance records, image records, the work list of the first
 * launch) goes up in one copy. The first launch sets every (image, triangle) up once into a screen record (64 bytes)
 * of a device block; the second walks the records per tile. The input block, the record block and, in host mode, a
 * staging block for the images are made by the group's first ar job, replaced when outgrown and counted in
 * svo_ctx_get_memory (svo_memory.device_bytes). Host mode copies each run of consecutive named slots out in one
 * piece; device mode writes in place. A ctx that never asks for an ar picture allocates, launches and copies nothing
 * more. */
int svo_submit_export_ar(svo_ctx *ctx, const int *seqs, int n, const svo_ar_style *style, const svo_ar_mesh *meshes,
                         int n_meshes, const svo_ar_instance *instances, const int *first, int n_instances,
                         const svo_ar_dst *dst, int mem);
int svo_export_ar(svo_ctx *ctx, const int *seqs, int n, const svo_ar_style *style, const svo_ar_mesh *meshes,
                  int n_meshes, const svo_ar_instance *instances, const int *first, int n_instances,
                  const svo_ar_dst *dst, int mem);   /* submit + wait */
/* stage entry of the kernels: n images in the tracker's two launches (the second chunked when the diagnostic
 * SVO_AR_TABLE_TILES bounds the tile table). src[i].image: the background plane (device memory, any base address,
 * stride >= width, 1 .. 32768 pixels a side; its width x height is the output's). src[i].draws: HOST array of
 * n_draws instanced meshes whose vertices, triangles and rgb (or NULL) are DEVICE memory, 4-byte aligned; a triangle
 * with a vertex index out of range is dropped and the top byte of a colour in `rgb` is ignored. At most SVO_AR_MAX_TRIANGLES triangles per image (SVO_ERR_CAPACITY).
 * Image i is seen through cameras[i] and goes to pixels + offset[i] (host array, >= 0, multiples of 4; pixels:
 * device, 4-byte aligned), rows dense. Exactly the images' bytes are written. Complete on return. */
typedef struct svo_ar_draw {          /* 88 bytes */
    float    model[12];
    const float   *vertices;
    const int32_t *triangles;
    const uint32_t *rgb;
    int32_t  n_vertices, n_triangles;
    uint32_t rgb_all;                 /* the instance's colour                                               */
    int32_t  _reserved;               /* 0                                                                   */
} svo_ar_draw;
typedef struct svo_ar_src {
    svo_image image;
    const svo_ar_draw *draws;
    int32_t n_draws;
    int32_t _reserved;                /* 0                                                                   */
} svo_ar_src;
int svo_render_ar(svo_handle *h, int n, const svo_ar_src *src, const svo_ar_camera *cameras, const int64_t *offset,
                  const svo_ar_style *style, uint8_t *pixels);

/* ---- dense: disparity and depth maps of many slots in one queued job ------------
 * The tracker computes stereo disparity at its keypoints only. A dense map is the reference's disparity search
 * (DepthFilter::calculate_disparities, src/lib/depth_filter.cpp:259-327, i.e. svo_ssd_disparity with clamp_half = 1)
 * evaluated at every point of a lattice over the rectified, converted left and right planes of a slot, which exist in
 * device memory only. A disparity job is the batched reader: the groups that own a named slot compute one map per
 * slot with one kernel launch each (dense.hip) and deliver it into host or device memory; the host writes one
 * svo_disparity_segment per named slot.
 *
 * Lattice: cols = W / step, rows = H / step (integer division); lattice point (ix, iy) is the pixel
 * x = ix * step + step / 2, y = iy * step + step / 2, and its value is exactly what
 * svo_ssd_disparity(left, right, {(x, y)}, 1, win, search_x, search_y, 1, .) gives for that point.
 *
 * Point rule: with wb = win / 2, wa = (win + 1) / 2,
 *   template box  x11 = max(0, x - wb), x12 = min(W - 1, x + wa), y11 = max(0, y - wb), y12 = min(H, y + wa)
 *   region box    x21 = x11, x22 = min(W - 1, x + wa + search_x), y21 = max(0, y - wb - search_y),
 *                 y22 = min(H - 1, y + wa + search_y)
 *   invalid (-1)  x12 <= 0, y12 <= 0, x11 >= W - 1 or y11 >= H - 1; the same four tests on the region box; or any of
 *                 tw = x12 - x11, th = y12 - y11, mw = (x22 - x21) - tw + 1, mh = (y22 - y21) - th + 1 is <= 0
 *   candidate     (k, j), 0 <= k < mh, 0 <= j < mw, has the exact integer
 *                 SSD(k, j) = sum over r < th, c < tw of (R[y21 + k + r][x21 + j + c] - L[y11 + r][x11 + c])^2,
 *                 rounded once to float
 * The clipping is the reference's own: the template never holds the last column, a template clipped at the bottom
 * leaves mh = y11 - y21, and near the right edge mw shrinks to 1.
 *
 * Argmin and ties, as one pass over the candidates in row-major order (k outer, j inner): a float value strictly
 * below the best so far sets best, minx = j, sum = j, count = 1; a value equal to the best with j >= minx adds j to
 * sum and 1 to count. d = (float)sum / (float)count, and the disparity is d < 0.5f ? 0.5f : d. (This equals the
 * reference's two loops: the first minimum of the float map, then the mean column over j >= minx, k >= miny.)
 *
 * Planes: the value plane is cols x rows float32, dense. SVO_DENSE_DISPARITY: the disparity as above.
 * SVO_DENSE_DEPTH: z = baseline / disparity of a valid point in float (outlier_check's _z; a valid disparity is
 * already >= 0.5) and 0 at an invalid point; baseline is that of the slot's rig. With style.cost = 1 a second plane
 * follows the first at + cols * rows * 4 bytes: best, the float-rounded minimum SSD, and -1 at an invalid point.
 *
 * Layout: image_bytes = planes * cols * rows * 4 rounded up to a multiple of 256; named slot i of a job goes to
 * offset = i * image_bytes of dst->values, whatever group owns it. Of a slot exactly the planes' bytes are written; a
 * slot whose status is SVO_DISPARITY_NONE writes only its segment. */
enum { SVO_DENSE_DISPARITY = 0, SVO_DENSE_DEPTH = 1 };
enum { SVO_DISPARITY_OK = 0,
       SVO_DISPARITY_NONE = 1 };    /* an empty slot, no keyframe yet, or the keyframe has given its image set back */

typedef struct svo_disparity_style {   /* 32 bytes; what one job computes; copied at submit                 */
    int32_t value;                  /* SVO_DENSE_*                                                          */
    int32_t step;                   /* 1 .. 16                                                              */
    int32_t win, search_x, search_y;/* 0: the ctx's window_size_depth_calculator / search_x / search_y; else within
                                       what svo_ssd_disparity accepts (win <= 35, search_x <= 64, search_y <= 8) */
    int32_t cost;                   /* 0 / 1: the second plane                                              */
    int32_t _reserved[2];           /* 0                                                                    */
} svo_disparity_style;

typedef struct svo_disparity_segment { /* 64 bytes, host, one per named slot                                */
    int32_t seq, run;               /* slot and ordinal of its run (svo_run_info.run)                       */
    int32_t frame_id;               /* of the slot's current frame; -1: empty slot                          */
    int32_t keyframe_id;            /* LAST_KEYFRAMES: the keyframe used (-1: the slot has none); FRAMES: -1 */
    int32_t status;                 /* SVO_DISPARITY_*                                                      */
    int32_t _pad;
    int64_t offset;                 /* the planes are bytes [offset, offset + planes * cols * rows * 4) of dst->values */
    float   pose[6];                /* FRAMES: svo_get_pose; LAST_KEYFRAMES: the keyframe's pose            */
    float   time_stamp;             /* of the slot's current frame                                          */
    float   baseline;               /* of the slot's rig                                                    */
} svo_disparity_segment;

typedef struct svo_disparity_dst {
    svo_disparity_segment *segments;/* HOST memory always, >= n entries                                     */
    float  *values;                 /* host or device (mem); 16-byte aligned                                */
    int64_t capacity;               /* bytes `values` holds                                                 */
} svo_disparity_dst;

/* the shape of one slot's planes of a job with that style in a ctx of these settings, without a GPU (any out pointer
 * may be NULL); planes is 1 or 2. Settings svo_ctx_create rejects, or a style a job rejects: SVO_ERR_INVALID */
int svo_disparity_size(const svo_camera_settings *cam, int width, int height, const svo_disparity_style *style,
                       int *cols, int *rows, int *planes, int64_t *image_bytes);
/* what: SVO_EXPORT_FRAMES (level 0 of the left pyramid and the right image of the slot's current frame; a slot that
 * sat steps out uses its last frame) or SVO_EXPORT_LAST_KEYFRAMES (the image set of the newest keyframe; once it has
 * given its images back the status is SVO_DISPARITY_NONE). These are the planes a view job shows for plane = LEFT,
 * level = 0 and plane = RIGHT: after rectification and colour conversion, and under SVO_MEM_DEVICE_BORROW the
 * caller's buffers, which the validity rule above keeps alive. Queued exactly as svo_submit_export_views is (seqs ==
 * NULL names every slot in order, n is ignored): the job sees every frame set, restart, load and pose update
 * submitted before it and none submitted after, only groups that own a named slot get work, no group waits for
 * another, the slot is not changed (its deferred pose-filter update is flushed first). style and dst are copied;
 * segments and values stay valid until svo_wait, after which everything is delivered. mem: SVO_MEM_HOST or
 * SVO_MEM_DEVICE, of `values`.
 * Rejected with SVO_ERR_INVALID and nothing queued: a slot out of range or named twice; a bad what, mem, value, cost
 * or step; a window or search value outside the limits; cols or rows of 0; a _reserved != 0; NULL segments; values
 * NULL or not 16-byte aligned; a failed ctx, as in svo_submit_images. SVO_ERR_CAPACITY: dst->capacity < named slots *
 * image_bytes (the bound, so it is checked here).
 * Host mode: a group computes its named slots densely into a device staging block, made by the group's first
 * host-mode disparity job and replaced when outgrown (svo_memory.device_bytes), and copies each run of consecutive
 * named slots out in one piece. Device mode writes in place and allocates nothing. A ctx that never asks for a
 * disparity map allocates, launches and copies nothing more. */
int svo_submit_export_disparity(svo_ctx *ctx, int what, const int *seqs, int n, const svo_disparity_style *style,
                                const svo_disparity_dst *dst, int mem);
int svo_export_disparity(svo_ctx *ctx, int what, const int *seqs, int n, const svo_disparity_style *style,
                         const svo_disparity_dst *dst, int mem);   /* submit + wait */
/* stage entry of the kernel: n image pairs in the job's launch (chunked when the diagnostic SVO_DENSE_TABLE_IMAGES
 * bounds the image table). src[i].left / right: gray planes of one size (device memory, any base address, stride >=
 * width, 1 .. 32768 pixels a side); the pairs of one call may differ in size. style->win, search_x and search_y must
 * be given (1 .. 35, 0 .. 64, 0 .. 8); cols or rows of 0 for an image is rejected. The planes of pair i go to
 * (char *)values + offset[i] (host array, >= 0, multiples of 16; values: device, 16-byte aligned). Exactly the
 * planes' bytes are written. Complete on return. */
typedef struct svo_dense_src {
    svo_image left, right;
    float     baseline;               /* SVO_DENSE_DEPTH: z = baseline / disparity                           */
    int32_t   _reserved;              /* 0                                                                   */
} svo_dense_src;
int svo_dense_disparity(svo_handle *h, int n, const svo_dense_src *src, const int64_t *offset,
                        const svo_disparity_style *style, float *values);

/* ---- clouds: dense coloured point clouds of many slots in one queued job ------------
 * A dense map ("dense" above) lives in image space; every consumer of this library's maps (the viewer reply, the
 * scene, svo_export_map) carries svo_map_point records in the world frame. A cloud job is the 3-D form of the dense
 * map: every lattice point becomes the kps3d the reference would give a new keypoint at that pixel
 * (DepthCalculator::calculate_depth, src/lib/depth_calculator.cpp:241-256; kf_init_kernel), bit for bit, is filtered,
 * coloured from the left plane and delivered as an svo_map_point, into host or device memory. Everything it needs
 * (the rectified, converted planes, the slot's rig, the tracked pose) is on the device and nowhere else.
 *
 * Lattice: cols = W / step, rows = H / step, pixel x = ix * step + step / 2, y = iy * step + step / 2. For a lattice
 * point, disp and best are exactly the two planes that a disparity job with value = SVO_DENSE_DISPARITY, cost = 1 and
 * the same step, win, search_x, search_y gives (-1: an invalid point). The window and search defaults, the point rule
 * and the argmin are those of "dense".
 *
 * Triangulation, in float32, every operation rounded once (no fused multiply-add), with the slot's rig fx, fy, cx, cy,
 * baseline and a pose (x, y, z, rx, ry, rz):
 *   _z = baseline / fmaxf(0.5f, disp);  _x = ((float)x - cx) / fx * _z;  _y = ((float)y - cy) / fy * _z
 *   SVO_CLOUD_WORLD:  p = R * (_x, _y, _z) + t, with R = (float)Rodrigues(rx, ry, rz) computed in double and each row
 *                     summed as s = 0; s += R[i][k] * v[k], k = 0, 1, 2 (PoseManager's float rotation matrix)
 *   SVO_CLOUD_CAMERA: p = (_x, _y, _z)
 *
 * Filter: an invalid point is always dropped. A valid point is dropped if any of
 *   disp < min_disparity;   _z > max_depth;   best > max_mean_cost * (float)(tw * th)
 * holds, each one float32 comparison (the product rounded once); a filter value of 0 is off. tw, th: the clipped
 * template box of the point rule (x12 - x11, y12 - y11).
 *
 * Record: one svo_map_point, 16 bytes: x, y, z = p's bits; color[0 .. 2] = L[y][x], the gray of the left plane;
 * flags = 0.
 *
 * Layouts. points_per_slot = cols * rows; named slot i of a job owns records [i * points_per_slot, (i + 1) *
 * points_per_slot) of dst->points, whatever group owns it.
 *   SVO_CLOUD_COMPACT:   the kept points of a slot lie densely in row-major lattice order (iy outer, ix inner) from
 *                        the slot's first record on: n_points records. The order is stable (two runs give the same
 *                        bytes) and nothing beyond record n_points is written.
 *   SVO_CLOUD_ORGANIZED: every lattice point has its record at iy * cols + ix. A dropped or invalid point gets
 *                        x = y = z = +0.0f, the gray and flags = SVO_CLOUD_DROPPED (no SVO_IGNORE_* bit); n_points is
 *                        still the kept count. */
enum { SVO_CLOUD_WORLD = 0, SVO_CLOUD_CAMERA = 1 };
enum { SVO_CLOUD_COMPACT = 0, SVO_CLOUD_ORGANIZED = 1 };
enum { SVO_CLOUD_OK = 0,
       SVO_CLOUD_NONE = 1 };        /* as SVO_DISPARITY_NONE: only the segment is written                   */
enum { SVO_CLOUD_DROPPED = 0x80 };  /* svo_map_point.flags of a dropped point in the organized layout       */

typedef struct svo_cloud_style {    /* 48 bytes; what one job computes; copied at submit                    */
    int32_t step;                   /* 1 .. 16                                                              */
    int32_t win, search_x, search_y;/* as in svo_disparity_style; 0: the ctx's settings                     */
    int32_t frame;                  /* SVO_CLOUD_WORLD / SVO_CLOUD_CAMERA                                   */
    int32_t layout;                 /* SVO_CLOUD_COMPACT / SVO_CLOUD_ORGANIZED                              */
    float   min_disparity;          /* the three filter values: finite, >= 0; 0: off                        */
    float   max_depth;
    float   max_mean_cost;
    int32_t _reserved[3];           /* 0                                                                    */
} svo_cloud_style;

typedef struct svo_cloud_segment {  /* 64 bytes, host, one per named slot                                   */
    int32_t seq, run;               /* slot and ordinal of its run (svo_run_info.run)                       */
    int32_t frame_id;               /* of the slot's current frame; -1: empty slot                          */
    int32_t keyframe_id;            /* LAST_KEYFRAMES: the keyframe used (-1: the slot has none); FRAMES: -1 */
    int32_t status;                 /* SVO_CLOUD_*                                                          */
    int32_t n_points;               /* kept points (0 with SVO_CLOUD_NONE)                                  */
    int64_t first_point;            /* the slot's records start at dst->points[first_point]                 */
    float   pose[6];                /* the pose used. FRAMES: svo_get_pose; LAST_KEYFRAMES: the keyframe's  */
    float   time_stamp;             /* of the slot's current frame                                          */
    float   baseline;               /* of the slot's rig                                                    */
} svo_cloud_segment;

typedef struct svo_cloud_dst {
    svo_cloud_segment *segments;    /* HOST memory always, >= n entries                                     */
    svo_map_point     *points;      /* host or device (mem); 16-byte aligned                                */
    int64_t            capacity;    /* records `points` holds                                               */
} svo_cloud_dst;

/* the lattice of one slot of a job with that style in a ctx of these settings, without a GPU (any out pointer may be
 * NULL). Settings svo_ctx_create rejects, or a style a job rejects: SVO_ERR_INVALID */
int svo_cloud_size(const svo_camera_settings *cam, int width, int height, const svo_cloud_style *style, int *cols,
                   int *rows, int64_t *points_per_slot);
/* what, seqs, n, mem, the planes read, the queueing and the lifetime of style, dst, segments and points: exactly as
 * svo_submit_export_disparity. The job sees every frame set, restart, load and pose update submitted before it and
 * none submitted after; only groups that own a named slot get work; the slot is not changed.
 * Rejected with SVO_ERR_INVALID and nothing queued: everything svo_submit_export_disparity rejects (points in the
 * place of values); a bad frame or layout; a filter value that is negative or not finite. SVO_ERR_CAPACITY:
 * dst->capacity < named slots * points_per_slot (the bound, so it is checked here).
 * Memory: a group searches into a staging block of its own (not the disparity job's), made by the group's first cloud
 * job and replaced when outgrown (svo_memory.device_bytes). Per named slot of the group it holds the disparity and
 * cost planes, the tile counts, the pose's matrices and the kept count, and in host mode the slot's records:
 *   slot_bytes = up256(2 * 4 * points_per_slot) + up256(4 * ceil(points_per_slot / 256)) + 256 + (host ? 16 * points_per_slot : 0)
 *   block      = min(named slots of the group, chunk) * slot_bytes + up256(4 * min(named slots of the group, chunk))
 * with up256 rounding up to a multiple of 256 and chunk = max(1, 256 MiB / slot_bytes) (the diagnostic
 * SVO_CLOUD_CHUNK_SLOTS lowers it): a job with more slots runs in chunks of so many. Host mode copies out each
 * slot's kept prefix (compact) or runs of consecutive slots (organized); the kept counts of a chunk come back in one
 * copy. A ctx that never asks for a cloud allocates, launches and copies nothing more. */
int svo_submit_export_cloud(svo_ctx *ctx, int what, const int *seqs, int n, const svo_cloud_style *style,
                            const svo_cloud_dst *dst, int mem);
int svo_export_cloud(svo_ctx *ctx, int what, const int *seqs, int n, const svo_cloud_style *style,
                     const svo_cloud_dst *dst, int mem);   /* submit + wait */
/* stage entry of the kernels: n image pairs (chunked when the diagnostic SVO_CLOUD_TABLE_IMAGES bounds the image
 * table). src[i].left / right as in svo_dense_src; the pairs of one call may differ in size. style->win, search_x and
 * search_y must be given. The records of pair i start at points[first[i]] (host array, >= 0; points: device, 16-byte
 * aligned): n_points of them in the compact layout, cols * rows in the organized one; nothing else is written.
 * counts: device int32[n], the kept count of every pair, or NULL. Complete on return. */
typedef struct svo_cloud_src {       /* 96 bytes */
    svo_image left, right;
    float     baseline, fx, fy, cx, cy;
    float     pose[6];                /* SVO_CLOUD_WORLD: x, y, z, rx, ry, rz                                 */
    int32_t   _reserved;              /* 0                                                                   */
} svo_cloud_src;
int svo_cloud_points(svo_handle *h, int n, const svo_cloud_src *src, const int64_t *first, const svo_cloud_style *style,
                     svo_map_point *points, int32_t *counts);

/* ---- cross-check: which values of a dense map or cloud to trust ------------
 * "dense" and "clouds" deliver the one-directional search at every lattice point, so they hold a confident-looking
 * value where the stereo pair has none: half-occluded bands beside depth edges, repeated texture, flat walls. A wrong
 * match in texture has a low cost, so neither the cost plane nor max_mean_cost sees it. The left-right consistency
 * check keeps a disparity only if the search from the matched right pixel back into the left image comes home. The
 * reverse search is the point rule of "dense" on the mirrored, swapped planes, which exist on the device only.
 *
 * Statement. point(L, R, x, y) is svo_ssd_disparity(L, R, {(x, y)}, 1, win, search_x, search_y, 1, .): the disparity
 * of "dense" (-1: invalid). With W the width, Lm[y][u] = R[y][W - 1 - u] and Rm[y][u] = L[y][W - 1 - u]. For the
 * lattice point at pixel (x, y) with disp its forward disparity (before any conversion to depth):
 *   lr = -1                      the point is invalid in the forward search; otherwise
 *   xr = x + (int)(disp + 0.5f)  (a float add rounded once, then truncation; disp >= 0.5)
 *   lr = -2                      xr > W - 1; otherwise
 *   rd = point(Lm, Rm, W - 1 - xr, y) with the same win, search_x, search_y
 *   lr = -2                      rd is invalid; else lr = fabsf(disp - rd)
 * A point FAILS at a tolerance max_lr_diff > 0 iff lr < 0.0f || lr > max_lr_diff (float32 comparisons).
 *
 * The setting rides beside the style in the "checked" form of each entry, which takes the unchecked entry's arguments
 * plus a check. With check == NULL or check->lr == 0 a checked entry is the unchecked one: the same launches, bytes,
 * memory, segments and rejections. Rejected with SVO_ERR_INVALID and nothing queued (a non-NULL check is checked
 * whatever its lr): lr other than 0 or 1, a negative or non-finite max_lr_diff, a non-zero _reserved; for a cloud
 * lr = 1 with max_lr_diff == 0. Everything else is rejected exactly as the unchecked entry rejects it.
 *
 * Disparity job and stage with lr = 1: a plane lr is appended, so the plane order is value, [cost], lr, planes is 2
 * or 3 and image_bytes = up256(planes * cols * rows * 4). With max_lr_diff > 0 the value plane of a failing point
 * gets the invalid value (-1 for SVO_DENSE_DISPARITY, 0 for SVO_DENSE_DEPTH); with max_lr_diff == 0 the check only
 * reports. The cost plane is never changed. SVO_DENSE_DEPTH is baseline / disp of the surviving disparity, the bits
 * of the unchecked job.
 * Cloud job and stage with lr = 1: a failing point is dropped, in addition to the three filters of "clouds"; order
 * and layouts are unchanged.
 *
 * Queueing: no new job kind. A checked job is a disparity or cloud job, so queue order, segments and the "slot is not
 * changed" rule are theirs.
 * Memory: the reverse search writes one float per column of every lattice row, reverse_bytes = up256(rows * W * 4) per
 * slot, into a staging block of the group (not the disparity or cloud job's), made by the group's first checked job
 * and replaced when outgrown (svo_memory.device_bytes):
 *   block = min(named slots of the group, chunk) * reverse_bytes
 * Disparity job: chunk = max(1, 256 MiB / reverse_bytes) (the diagnostic SVO_LR_CHUNK_SLOTS lowers it); the forward
 * search of all named slots runs as in the unchecked job, then the reverse search and the check run in chunks of so
 * many slots. The forward disparity is converted in place (a lane reads and writes only its own lattice point), so a
 * device-mode job with value = SVO_DENSE_DEPTH needs no copy of it. Cloud job: the chunk of "clouds" with slot_bytes +
 * reverse_bytes in the place of slot_bytes; the check masks the staged disparity plane before the count and write
 * launches, which therefore agree as before. An unchecked job allocates what it did; a ctx that never asks for a check
 * allocates, launches and copies nothing more. */
typedef struct svo_stereo_check {   /* 32 bytes; copied at submit */
    int32_t lr;            /* 0: off (the same as a NULL check), 1: on                       */
    float   max_lr_diff;   /* finite, >= 0; 0: report only (a cloud job requires > 0)        */
    int32_t _reserved[6];  /* 0 */
} svo_stereo_check;

/* svo_disparity_size of a checked job: planes is 1 .. 3 */
int svo_disparity_size_checked(const svo_camera_settings *cam, int width, int height, const svo_disparity_style *style,
                               const svo_stereo_check *check, int *cols, int *rows, int *planes, int64_t *image_bytes);
int svo_submit_export_disparity_checked(svo_ctx *ctx, int what, const int *seqs, int n, const svo_disparity_style *style,
                                        const svo_stereo_check *check, const svo_disparity_dst *dst, int mem);
int svo_export_disparity_checked(svo_ctx *ctx, int what, const int *seqs, int n, const svo_disparity_style *style,
                                 const svo_stereo_check *check, const svo_disparity_dst *dst, int mem);   /* submit + wait */
/* stage entry: svo_dense_disparity with the check; the reverse planes of a table chunk live in the handle's workspace */
int svo_dense_disparity_checked(svo_handle *h, int n, const svo_dense_src *src, const int64_t *offset,
                                const svo_disparity_style *style, const svo_stereo_check *check, float *values);
int svo_submit_export_cloud_checked(svo_ctx *ctx, int what, const int *seqs, int n, const svo_cloud_style *style,
                                    const svo_stereo_check *check, const svo_cloud_dst *dst, int mem);
int svo_export_cloud_checked(svo_ctx *ctx, int what, const int *seqs, int n, const svo_cloud_style *style,
                             const svo_stereo_check *check, const svo_cloud_dst *dst, int mem);   /* submit + wait */
/* stage entry: svo_cloud_points with the check */
int svo_cloud_points_checked(svo_handle *h, int n, const svo_cloud_src *src, const int64_t *first, const svo_cloud_style *style,
                             const svo_stereo_check *check, svo_map_point *points, int32_t *counts);

/* ---- sgm: semi-global aggregation and sub-pixel values for dense maps ------------
 * In "dense" a lattice point decides alone (winner takes all), so a flat wall gives noise, and its disparities are
 * whole numbers but for the tie mean. Semi-global matching cures both: the costs of "dense" are kept as a volume,
 * penalties for disparity changes are aggregated along four scanline paths over the lattice, the winner is taken from
 * the sum over the paths, and a parabola through the winner's neighbours gives the fraction. All of it is integer
 * arithmetic up to the last four float operations, and it is held to the bit like everything else here.
 *
 * Statement. The lattice, the boxes and the candidates (k, j) are those of "dense". D = search_x + 1 <= 64. For a
 * valid point count = mw and area = tw * th; for an invalid point count = 0.
 *   Cost volume  j < count:        C(p, j) = min(cost_cap, (min over k < mh of SSD(k, j)) / area), the exact integer
 *                                  SSD and the exact floor division
 *                count <= j < D:   C(p, j) = cost_cap
 *                invalid point:    C(p, j) = 0 for every j
 *   Paths        four directions r over the lattice: (+1, 0), (-1, 0), (0, +1), (0, -1) in (ix, iy).
 *                p - r outside the lattice:  L_r(p, j) = C(p, j)
 *                otherwise, with P = L_r(p - r, .) over all D entries and m = min over j of P(j):
 *                  L_r(p, j) = C(p, j) + min(P(j), P(j - 1) + p1 [j > 0], P(j + 1) + p1 [j < D - 1], m + p2) - m
 *                S(p, j) = sum over r of L_r(p, j). L_r <= cost_cap + p2, so S <= 4 * (cost_cap + p2) fits 16 bits.
 *   Value        an invalid point (count = 0) is -1, with SVO_DENSE_DEPTH 0.
 *                j0 = the smallest j < count with the least S(p, j);  d = (float)j0.
 *                With subpixel = 1 and 0 < j0 < count - 1, with the ints a = S(j0 - 1), b = S(j0), c = S(j0 + 1):
 *                  d = (float)j0 + (float)(a - c) / (float)(2 * (a - 2 * b + c))
 *                (the denominator is >= 2 because j0 is the first minimum; two exact conversions, one division and
 *                one addition, each rounded once to float).
 *                disparity = d < 0.5f ? 0.5f : d;  depth = baseline / disparity.
 *                With cost = 1 the second plane holds (float)S(p, j0), or -1 at an invalid point.
 * There are no defaults for p1, p2 and cost_cap in this ABI. */
typedef struct svo_sgm_params {     /* 32 bytes; copied at submit */
    int32_t paths;                  /* 4 (8 is reserved for the diagonals and rejected for now) */
    int32_t p1, p2;                 /* 1 <= p1 <= p2 */
    int32_t cost_cap;               /* >= 1; 4 * (cost_cap + p2) <= 65535 */
    int32_t subpixel;               /* 0 / 1 */
    int32_t _reserved[3];           /* 0 */
} svo_sgm_params;

/* The SGM mode of the disparity job: queued exactly as svo_submit_export_disparity is, and it rejects what that
 * rejects; also (SVO_ERR_INVALID, nothing queued) a NULL sgm, a bad field of it, and an effective search_x > 63. The
 * segments, the shape of a slot's planes and image_bytes are those of svo_disparity_size for the style; the value and
 * cost planes hold the values of the statement above. Inside the ctx it is the disparity job carrying the params, not
 * another kind of queue entry. Its cross-check is a rule of its own, "sgm cross-check" below.
 * Memory: the sums, the volume and the count plane of a slot (2 * cols * rows * D * 2 bytes and cols * rows * 2, each
 * rounded up to 256) live in a block of the group, made by the group's first SGM job and replaced when outgrown
 * (svo_memory.device_bytes). The slots of a job go through it in chunks of max(1, 512 MiB / slot bytes) slots (the
 * diagnostic SVO_SGM_CHUNK_SLOTS lowers it); one slot always fits. A 752 x 480 slot at step 1 with D = 61 needs 44 MB
 * for the volume and as much for the sums, at step 4 2.75 MB each. */
int svo_submit_export_disparity_sgm(svo_ctx *ctx, int what, const int *seqs, int n, const svo_disparity_style *style,
                                    const svo_sgm_params *sgm, const svo_disparity_dst *dst, int mem);
int svo_export_disparity_sgm(svo_ctx *ctx, int what, const int *seqs, int n, const svo_disparity_style *style,
                             const svo_sgm_params *sgm, const svo_disparity_dst *dst, int mem);   /* submit + wait */

/* Stage entries, over the handle's workspace; each complete on return. src, style and the lattice as in
 * svo_dense_disparity, but style->search_x <= 63 (SVO_ERR_INVALID beyond it).
 *
 * svo_dense_cost_volume: the cost volume alone. Pair i writes its volume, uint16 [rows][cols][D] (j fastest, dense), at
 * (char *)volumes + volume_offset[i] and its count plane, uint16 [rows][cols], at (char *)volumes + count_offset[i]
 * (host arrays, >= 0, multiples of 2; volumes: device, 2-byte aligned). This layout is part of the ABI. Exactly these
 * bytes are written. cost_cap: 1 .. 65535. style->value and cost are checked and not used. */
int svo_dense_cost_volume(svo_handle *h, int n, const svo_dense_src *src, const svo_disparity_style *style, int cost_cap,
                          const int64_t *volume_offset, const int64_t *count_offset, uint16_t *volumes);
/* svo_sgm_aggregate: paths and value rule over the caller's volumes in that layout (costs of any kind, census for
 * one). volumes[i] (host array of device pointers, 2-byte aligned): volume i; an entry above sgm->cost_cap is read as
 * cost_cap. counts: NULL, or a host array of device pointers to the count planes (a NULL entry, or counts == NULL:
 * every point has D candidates; a count above D is read as D). value: SVO_DENSE_*, cost: 0 / 1. The planes of volume i
 * go to (char *)values + offset[i] as in svo_dense_disparity. cols, rows >= 1, 1 <= D <= 64. The sums S of a chunk of
 * volumes live in the handle's workspace; a call is chunked so that a chunk's S stays within 256 MiB (the diagnostic
 * SVO_SGM_CHUNK_SLOTS lowers the volumes per chunk), one volume always fits, and a single volume whose S needs more
 * than 1 GiB is answered with SVO_ERR_CAPACITY. */
typedef struct svo_sgm_shape {      /* 16 bytes */
    int32_t cols, rows, D;
    float   baseline;               /* SVO_DENSE_DEPTH: z = baseline / disparity */
} svo_sgm_shape;
int svo_sgm_aggregate(svo_handle *h, int n, const svo_sgm_shape *shapes, const uint16_t *const *volumes,
                      const uint16_t *const *counts, int value, int cost, const svo_sgm_params *sgm, const int64_t *offset,
                      float *values);
/* svo_dense_disparity_sgm: the two together for pairs of any sizes: svo_dense_disparity's arguments and planes (shape
 * and bytes per pair as svo_disparity_size gives them for the style), the values those of the statement. The volume,
 * the count plane and S of a chunk of pairs live in the handle's workspace, chunked as above (volume, counts and S of a
 * chunk within 512 MiB); a single pair whose volume needs more than 1 GiB is answered with SVO_ERR_CAPACITY. */
int svo_dense_disparity_sgm(svo_handle *h, int n, const svo_dense_src *src, const int64_t *offset,
                            const svo_disparity_style *style, const svo_sgm_params *sgm, float *values);

/* ---- sgm cross-check: the left-right check of an SGM map, and clouds of SGM maps ------------
 * SGM fills a half-occluded band with smooth, confident, wrong values: the aggregated cost is low there and
 * max_mean_cost cannot see it. The check of "cross-check" asks a second, mirrored search; for an SGM map that second
 * search is a second SGM map, the same arithmetic run on the mirrored, swapped planes over their own lattice.
 *
 * Statement. With W the width, step, cols, rows and x = ix * step + step / 2 of "dense":
 *   fwd = the SGM disparity plane of (L, R) by the statement of "sgm" (always the disparity, before any conversion to
 *         depth);
 *   rev = the SGM disparity plane of (Lm, Rm), Lm[y][u] = R[y][W - 1 - u], Rm[y][u] = L[y][W - 1 - u], with the same
 *         style and params, over the lattice "dense" gives the mirrored planes: the same cols, rows and x.
 * For the lattice point (ix, iy) at pixel x with disp = fwd[iy][ix]:
 *   lr = -1                      disp is invalid; otherwise
 *   xr = x + (int)(disp + 0.5f)  (a float add rounded once, then truncation; disp >= 0.5)
 *   lr = -2                      xr > W - 1; otherwise
 *   ixm = min((W - 1 - xr) / step, cols - 1)  (integer division: the lattice cell of the mirrored pair that holds the
 *         matched column W - 1 - xr; the clamp bites only for step >= 5 with W % step >= 2 + step / 2)
 *   rd = rev[iy][ixm]
 *   lr = -2                      rd is invalid; else lr = fabsf(disp - rd)
 * Failing (lr < 0.0f || lr > max_lr_diff at max_lr_diff > 0), the lr plane, the invalid value of a failing point, the
 * untouched cost plane and SVO_DENSE_DEPTH = baseline / disp of a survivor are exactly as in "cross-check". With a
 * check the forward SGM run writes disparities and the check does the division, the float operation of the unchecked
 * SGM map: a point of a depth job that does not fail has the unchecked SGM job's bits.
 *
 * Entries: the SGM entry's arguments plus a svo_stereo_check. check == NULL or check->lr == 0 is the unchecked SGM
 * entry, launch for launch. Rejected (SVO_ERR_INVALID, nothing queued) is what the SGM entry rejects and what
 * "cross-check" rejects of a check, together; the shape of a slot's planes is that of svo_disparity_size_checked. No
 * new kind of queue entry: these are disparity and cloud jobs. The top-level check of "cross-check" stays what it is:
 * svo_submit_export_disparity_checked and svo_submit_export_cloud_checked run winner takes all.
 *
 * Clouds of SGM maps (svo_submit_export_cloud_sgm; check NULL or lr == 0: no check; a check needs max_lr_diff > 0):
 * the cloud job of "clouds" with the SGM value plane (the disparity, cost = 1) as its staged disparity plane and
 * best = (float)S(p, j0) as its cost plane. Triangulation, layouts, min_disparity and max_depth are unchanged;
 * max_mean_cost != 0 drops a point iff best > max_mean_cost * 4.0f (one float product, one comparison): S is the sum
 * over four paths of a cost that is per pixel already, so the factor is the number of paths where "clouds" has the
 * template's area. With a check the check masks the staged disparity plane before the count and write launches.
 * Shapes are those of svo_cloud_size. Also rejected: an effective search_x > 63, a NULL or bad sgm.
 *
 * Memory. A checked SGM slot stages two volumes, two blocks of sums, two count planes and the reverse plane:
 *   slot_bytes = 2 * (2 * up256(cols * rows * D * 2) + up256(cols * rows * 2)) + up256(cols * rows * 4)
 * in the block of "sgm" (svo_memory.device_bytes), with the same chunk rule: chunks of max(1, 512 MiB / slot_bytes) slots
 * (SVO_SGM_CHUNK_SLOTS lowers it), block = min(delivered slots of the group, chunk) * slot_bytes; one slot always
 * fits. An unchecked SGM slot is 2 * up256(cols * rows * D * 2) + up256(cols * rows * 2) as before. A checked SGM job
 * does not use the reverse block of "cross-check". An SGM cloud job stages what a cloud job stages (slot_bytes of
 * "clouds", no reverse_bytes) plus this block for the slots of one of its chunks. An unchecked SGM job, a checked or
 * unchecked winner-takes-all job and a ctx that uses none of this allocate, launch and copy what they did.
 *
 * Launches of a chunk of m checked slots: the cost volumes of the m pairs, those of the m mirrored pairs, the two
 * launches of the paths over one table of 2 m volumes (the mirrored ones behind the forward ones, writing their
 * disparity alone), and the lattice form of the check kernel. */
int svo_submit_export_disparity_sgm_checked(svo_ctx *ctx, int what, const int *seqs, int n, const svo_disparity_style *style,
                                            const svo_sgm_params *sgm, const svo_stereo_check *check,
                                            const svo_disparity_dst *dst, int mem);
int svo_export_disparity_sgm_checked(svo_ctx *ctx, int what, const int *seqs, int n, const svo_disparity_style *style,
                                     const svo_sgm_params *sgm, const svo_stereo_check *check, const svo_disparity_dst *dst,
                                     int mem);   /* submit + wait */
/* stage entry: svo_dense_disparity_sgm with the check; per pair the workspace also holds the mirrored pair's volume,
 * count plane, S and disparity plane (chunked as there, within 512 MiB) */
int svo_dense_disparity_sgm_checked(svo_handle *h, int n, const svo_dense_src *src, const int64_t *offset,
                                    const svo_disparity_style *style, const svo_sgm_params *sgm,
                                    const svo_stereo_check *check, float *values);
int svo_submit_export_cloud_sgm(svo_ctx *ctx, int what, const int *seqs, int n, const svo_cloud_style *style,
                                const svo_sgm_params *sgm, const svo_stereo_check *check, const svo_cloud_dst *dst, int mem);
int svo_export_cloud_sgm(svo_ctx *ctx, int what, const int *seqs, int n, const svo_cloud_style *style,
                         const svo_sgm_params *sgm, const svo_stereo_check *check, const svo_cloud_dst *dst,
                         int mem);   /* submit + wait */
/* stage entry: svo_cloud_points over SGM maps (style->win, search_x, search_y given; search_x <= 63) */
int svo_cloud_points_sgm(svo_handle *h, int n, const svo_cloud_src *src, const int64_t *first, const svo_cloud_style *style,
                         const svo_sgm_params *sgm, const svo_stereo_check *check, svo_map_point *points, int32_t *counts);

/* ---- scene clouds: dense clouds ("clouds", "cross-check") drawn in the scene picture ------------
 * A scene job can draw, beside the elements above, svo_map_point records: the dense cloud of each named slot's frame
 * or newest keyframe (the LIVE LAYER), records of the caller's in device memory (the EXTRA SPAN), or both.
 *
 * The picture. A CLOUD POINT is a svo_map_point record (x, y, z, color[3], flags). It is drawn unless
 * flags & SVO_CLOUD_DROPPED or flags & style->filter.drop_flags (own_only and min_inliers do not apply: a record has
 * neither). It follows the `point` rule of "scene" word for word with s = clouds->point_size (the stage entry: its
 * point_size argument): c = T(x, y, z); dropped unless every c_k is finite and c_2 >= near; u = (f * c_0) / c_2 + cx,
 * v = (f * c_1) / c_2 + cy; dropped unless |u| < 2^15 and |v| < 2^15; px = floor(u), py = floor(v); it covers the
 * s x s pixels [px - (s-1)/2, px - (s-1)/2 + s - 1] x [py - (s-1)/2, py - (s-1)/2 + s - 1]. Its depth is c_2, its
 * colour color[0], color[1], color[2] as r, g, b, its class SVO_SCENE_CLASS_CLOUD = 4:
 *   key = bits(c_2) << 32 | 4 << 24 | r << 16 | g << 8 | b
 * so at equal depth a keypoint (class 3) and every line beat a cloud point, and between two cloud points the smaller
 * colour word wins. No key of "scene" changes: a picture without cloud points is byte for byte the picture of "scene".
 *
 * How it is drawn (scene.hip): a splat pass visits every record once, one lane per record, and offers its key with a
 * 64-bit atomic min to a key plane uint64[rows][cols] of its image in device memory, cleared to all ones before; the
 * tile kernel then starts from that plane instead of from all ones. The min is an integer min, so the bytes depend on
 * no order and two runs agree.
 *
 * The job. svo_submit_export_scenes_clouds is svo_submit_export_scenes with a svo_scene_clouds. No new job kind: queue
 * order, segments, "the slot is not changed", the SVO_SCENE_NONE rule (such a slot draws nothing; its info is status =
 * SVO_CLOUD_NONE, keyframe_id = -1, live_points = 0 and the span's n) and the copy-out are the scene job's. clouds == NULL, or live == 0
 * with extra == NULL, IS svo_submit_export_scenes: the same launches, bytes, memory and rejections.
 *   live layer  per named slot exactly the records that svo_submit_export_cloud_checked(what, ..., `cloud` with
 *               layout = SVO_CLOUD_ORGANIZED, check, ...) delivers for that slot at the same queue position: the same
 *               planes, rig and pose, the same launches, bit for bit. They go into a staging block of the group and
 *               are never copied out. A slot the cloud job gives SVO_CLOUD_NONE (LAST_KEYFRAMES without a keyframe)
 *               shows the picture without a live layer.
 *   extra span  extra[i] belongs to seqs[i]: n records in device memory, read when the job runs (they stay valid and
 *               unchanged until svo_wait). A caller shows an accumulated map this way: it keeps compact clouds of
 *               earlier keyframes, or a svo_export_map result, in one device array and passes it with every job.
 *   info[i]     of seqs[i]: status mirrors SVO_CLOUD_OK / SVO_CLOUD_NONE of the live layer (NONE with live == 0),
 *               keyframe_id is the cloud segment's (-1 without a live layer), live_points its kept count,
 *               extra_points the span's n.
 * Rejected with SVO_ERR_INVALID and nothing queued: everything svo_submit_export_scenes rejects; with live == 1
 * everything svo_submit_export_cloud_checked rejects of `cloud` and `check`, cloud.frame != SVO_CLOUD_WORLD,
 * cloud.layout != 0, a bad `what`; live other than 0 or 1; point_size outside 1 .. 16; a non-zero _reserved; a span
 * with n < 0, or with n > 0 and a NULL or not 16-byte aligned pointer.
 * Memory, per group, in blocks of its own made by the first such job, replaced when outgrown and counted in
 * svo_memory.device_bytes:
 *   key planes   key_bytes = up256(8 * cols * rows) per slot of a chunk
 *   live layer   16 * points_per_slot per slot of a chunk, beside what the cloud job itself stages in device mode:
 *                its slot_bytes ("clouds") and, checked, reverse_bytes ("cross-check"), in the cloud job's blocks
 *   block        min(named slots of the group, chunk) * (key_bytes + 16 * points_per_slot [live])
 *   chunk        max(1, 256 MiB / (key_bytes + [live: slot_bytes + 16 * points_per_slot + reverse_bytes])); the
 *                diagnostic SVO_SCENE_CHUNK_SLOTS lowers it
 * Per chunk the order on the group's stream is: search, check, cloud write, clear, splat, tile render. The span table
 * (pieces of 1024 records, one workgroup each) goes through the group's argument blocks like the tile table; the
 * diagnostic SVO_SCENE_TABLE_SPANS makes it smaller. A job without clouds allocates what it did. */
enum { SVO_SCENE_CLASS_CLOUD = 4 };

typedef struct svo_scene_span {       /* 16 bytes */
    const svo_map_point *points;      /* device, 16-byte aligned                                             */
    int64_t n;                        /* >= 0 records                                                        */
} svo_scene_span;

typedef struct svo_scene_cloud_info { /* 32 bytes, host, one per named slot                                  */
    int32_t status;                   /* SVO_CLOUD_OK: a live cloud was drawn; SVO_CLOUD_NONE                */
    int32_t keyframe_id;              /* LAST_KEYFRAMES: the keyframe used; else -1                          */
    int32_t live_points;              /* the live layer's kept count                                         */
    int32_t _pad;
    int64_t extra_points;             /* the extra span's n                                                  */
    int64_t _pad2;
} svo_scene_cloud_info;

typedef struct svo_scene_clouds {     /* copied at submit (the spans too; not the records)                   */
    int32_t live;                     /* 0: no live layer, 1: the dense cloud of `what` of each named slot   */
    int32_t what;                     /* SVO_EXPORT_FRAMES / SVO_EXPORT_LAST_KEYFRAMES                       */
    svo_cloud_style  cloud;           /* frame SVO_CLOUD_WORLD, layout 0; step, window, search, the filters  */
    svo_stereo_check check;           /* as in svo_submit_export_cloud_checked                               */
    int32_t point_size;               /* 1 .. 16                                                             */
    int32_t _reserved[3];             /* 0                                                                   */
    const svo_scene_span *extra;      /* NULL, or ONE PER NAMED SLOT (n = 0: none)                           */
    svo_scene_cloud_info *info;       /* NULL, or host, one per named slot; valid until svo_wait             */
} svo_scene_clouds;

int svo_submit_export_scenes_clouds(svo_ctx *ctx, const int *seqs, int n, const svo_scene_style *style,
                                    const svo_scene_clouds *clouds, const svo_scene_camera *cameras,
                                    const svo_scene_dst *dst, int mem);
int svo_export_scenes_clouds(svo_ctx *ctx, const int *seqs, int n, const svo_scene_style *style,
                             const svo_scene_clouds *clouds, const svo_scene_camera *cameras,
                             const svo_scene_dst *dst, int mem);   /* submit + wait */
/* stage entry: svo_render_scene with cloud points. Image i also shows the n_spans[i] spans that follow those of image
 * i - 1 in `spans` (host arrays; n_spans[i] >= 0; spans may be NULL if every count is 0), as cloud points of
 * `point_size`. The key planes of the images that have a record live in the handle's workspace; the span table is
 * chunked when the diagnostic SVO_SCENE_TABLE_SPANS bounds it. With no record anywhere it is svo_render_scene: the
 * same launches and bytes. Rejected as svo_render_scene rejects, and: point_size outside 1 .. 16, a negative count, a
 * span with n < 0 or with n > 0 and a NULL or not 16-byte aligned pointer. Complete on return. */
int svo_render_scene_clouds(svo_handle *h, int n, const svo_scene_src *src, const svo_scene_span *spans,
                            const int32_t *n_spans, const svo_scene_camera *cameras, const int64_t *offset,
                            const svo_scene_style *style, int32_t point_size, uint8_t *pixels);

/* ---- ar occlusion: meshes of the AR picture hidden behind the scene's dense stereo depth ------------
 * "ar" draws its meshes over the camera image as if the room were empty: a box placed behind a table leg is painted
 * over the leg. The checked cloud of the very frame the picture shows ("clouds", "cross-check"; frame =
 * SVO_CLOUD_CAMERA) is a depth of the left rectified plane in the camera frame of the picture's depth c_2, so one
 * comparison per pixel decides whether the scene is in front of the mesh.
 *
 * An OCCLUDER of an image is a lattice of svo_map_point records in the SVO_CLOUD_ORGANIZED layout: cols, rows, step,
 * the record of lattice point (ix, iy) at iy * cols + ix. Only z and flags of a record are read.
 *   occluder of a pixel   pixel (px, py) of the picture belongs to cell ix = px / step, iy = py / step (integer
 *              division). The pixel HAS AN OCCLUDER DEPTH zo = record.z iff ix < cols and iy < rows, the record's
 *              flags carry neither SVO_CLOUD_DROPPED nor any bit of drop_flags, and zo is finite and > 0. Otherwise
 *              nothing occludes the pixel: so also in the columns and rows beyond cols * step, rows * step when step
 *              does not divide the size, and everywhere in an image without an occluder (records == NULL).
 *   pixel      the rule of "ar" extended, not changed: the keys, the coverage and the smallest-key winner are those of
 *              "ar". Let z be the winner's depth, the float whose bits are key >> 32. The winner is HIDDEN iff the
 *              pixel has an occluder depth and z > zo + margin: one float32 add rounded once, one float32 comparison
 *              (zo + margin = +inf hides nothing). A pixel without a winner shows the background as before. Testing
 *              only the winner is the same as testing every fragment: every other covering triangle of the pixel has
 *              z' >= z (the key orders by depth first), so it is hidden whenever the winner is, and when the winner is
 *              visible it wins whatever becomes of the others.
 *   hidden     SVO_AR_HIDDEN_DROP: a hidden pixel shows the background (g, g, g).
 *              SVO_AR_HIDDEN_DIM:  every channel becomes (c' * (256 - a) + g * a + 128) >> 8 in integers, with a =
 *              alpha (0 .. 256), c' the winner's shaded channel and g the background gray: a = 0 shows the mesh
 *              unchanged, a = 256 the background.
 *   visibility per image, exact integers: covered = the pixels that have a winner, hidden = those of them whose winner
 *              is hidden. They are summed on the device with 64-bit integer atomic adds, one pair per workgroup after a
 *              reduction inside it, so the order of arrival cannot matter.
 *
 * The job. svo_submit_export_ar_occluded is svo_submit_export_ar with a svo_ar_occlusion. No new job kind: queue
 * order, segments, the SVO_AR_NONE rule (such a slot writes only its segment; its info is status = SVO_CLOUD_NONE and
 * zeros), the copy-out and "the slot is not changed" are the AR job's. occlusion == NULL or on == 0 IS
 * svo_submit_export_ar: the same launches, bytes and memory (of a non-NULL occlusion the scalar fields are checked
 * whatever its on; cloud, check and info are read with on == 1 only). With on == 1 named slot i's occluder is exactly the records that svo_submit_export_cloud_checked(
 * SVO_EXPORT_FRAMES, ..., `cloud` with frame = SVO_CLOUD_CAMERA and layout = SVO_CLOUD_ORGANIZED, check, ...) delivers
 * for that slot at the same queue position: the same planes, rig and launches, bit for bit, with cols = W / step,
 * rows = H / step. They go into a staging block of the group and never leave the device. The frame is always the
 * current frame: that is the image the picture shows. info[i] of named slot i: status = SVO_CLOUD_OK and
 * occluder_points = the cloud's kept count where a picture was drawn, covered and hidden as above.
 * Rejected with SVO_ERR_INVALID and nothing queued: everything svo_submit_export_ar rejects; of a non-NULL occlusion
 * on or hidden outside their values, alpha outside 0 .. 256, a margin that is negative or not finite, a non-zero
 * _reserved; with on == 1 everything svo_submit_export_cloud_checked rejects of `cloud` and `check`, cloud.frame !=
 * SVO_CLOUD_CAMERA, cloud.layout != 0; in the stage entry also an occluder with step outside 1 .. 16, with cols or rows <= 0, with a pointer that
 * is not 16-byte aligned or with a non-zero _reserved.
 * Memory, per group: the live layer has a block of its own, 16 * points_per_slot per slot of a chunk, made by the
 * group's first occluded job, replaced when outgrown and counted in svo_memory.device_bytes. It sits beside what the
 * cloud job itself stages in device mode in its own blocks (slot_bytes of "clouds" and, checked, reverse_bytes of
 * "cross-check"). chunk = max(1, 256 MiB / (slot_bytes + 16 * points_per_slot + reverse_bytes)); the diagnostic
 * SVO_AR_CHUNK_SLOTS lowers it. The input block of the AR job also carries one occluder entry (32 bytes) and one pair
 * of counters (16 bytes) per delivered slot. Per chunk the order on the group's stream is: search, check, cloud write,
 * set-up, tile render. The counters of all slots come back in the job's one copy, after the last chunk. An unoccluded
 * job allocates what it did; a ctx that never asks allocates, launches and copies nothing more. */
enum { SVO_AR_HIDDEN_DROP = 0, SVO_AR_HIDDEN_DIM = 1 };

typedef struct svo_ar_visibility {    /* 32 bytes, host, one per named slot / image                          */
    int32_t status;                   /* SVO_CLOUD_OK: the image had an occluder; SVO_CLOUD_NONE             */
    int32_t occluder_points;          /* the job: the cloud's kept count; the stage entry: 0                 */
    int64_t covered;                  /* pixels that have a winner                                           */
    int64_t hidden;                   /* those whose winner is hidden                                        */
    int64_t _pad;
} svo_ar_visibility;

typedef struct svo_ar_occlusion {     /* 128 bytes; copied at submit                                         */
    int32_t on;                       /* 0: the job IS svo_submit_export_ar; 1: occluded                     */
    int32_t hidden;                   /* SVO_AR_HIDDEN_DROP / SVO_AR_HIDDEN_DIM                              */
    int32_t alpha;                    /* 0 .. 256 (read by DIM only; checked always)                         */
    float   margin;                   /* finite, >= 0, in the unit of the depths                             */
    uint32_t drop_flags;              /* records with any of these flag bits occlude nothing                 */
    int32_t _reserved[3];             /* 0                                                                   */
    svo_cloud_style  cloud;           /* frame SVO_CLOUD_CAMERA, layout 0; step, window, search, the filters */
    svo_stereo_check check;           /* as in svo_submit_export_cloud_checked                               */
    svo_ar_visibility *info;          /* NULL, or host, one per named slot; valid until svo_wait             */
    int64_t _reserved2;               /* 0                                                                   */
} svo_ar_occlusion;

typedef struct svo_ar_occluder {      /* 24 bytes; one image of the stage entry                              */
    const svo_map_point *records;     /* device, 16-byte aligned, cols * rows records; NULL: no occluder     */
    int32_t cols, rows, step;         /* > 0, > 0, 1 .. 16 (not read with records == NULL)                   */
    int32_t _reserved;                /* 0                                                                   */
} svo_ar_occluder;

int svo_submit_export_ar_occluded(svo_ctx *ctx, const int *seqs, int n, const svo_ar_style *style,
                                  const svo_ar_occlusion *occlusion, const svo_ar_mesh *meshes, int n_meshes,
                                  const svo_ar_instance *instances, const int *first, int n_instances,
                                  const svo_ar_dst *dst, int mem);
int svo_export_ar_occluded(svo_ctx *ctx, const int *seqs, int n, const svo_ar_style *style,
                           const svo_ar_occlusion *occlusion, const svo_ar_mesh *meshes, int n_meshes,
                           const svo_ar_instance *instances, const int *first, int n_instances,
                           const svo_ar_dst *dst, int mem);   /* submit + wait */
/* stage entry: svo_render_ar plus one svo_ar_occluder per image (host array) and a host array of n visibilities, or
 * NULL. Only on, hidden, alpha, margin, drop_flags and the reserved words of the occlusion are read. With occlusion ==
 * NULL or on == 0 it is svo_render_ar: the same launches and bytes (occluders is not read; a visibility gets status =
 * SVO_CLOUD_NONE and zeros). The occluder table and the counters live in the handle's workspace, behind the tables of
 * svo_render_ar. Complete on return. */
int svo_render_ar_occluded(svo_handle *h, int n, const svo_ar_src *src, const svo_ar_camera *cameras,
                           const int64_t *offset, const svo_ar_style *style, const svo_ar_occlusion *occlusion,
                           const svo_ar_occluder *occluders, uint8_t *pixels, svo_ar_visibility *visibility);

/* ---- voxel maps: svo_map_point records fused into a sparse voxel grid ------------
 * "clouds" gives one cloud per frame or keyframe. A voxel map is what they add up to: a hash table in device memory,
 * bounded in size, that holds every surface once and averages the records that fell into the same voxel. It takes
 * svo_map_point records from anywhere (clouds, svo_export_map, a caller's own) and gives svo_map_point records back,
 * so every consumer of those reads it. The fusion is stated in integer arithmetic: integer adds, a max and the claim
 * of a key commute, so a map's content does not depend on the order of arrival and an extraction, which sorts by
 * key, gives the same bytes in every run. No float atomic is used.
 *
 * A map has a voxel edge `voxel` (float32, finite, > 0), capacity = 1 << log2_capacity entries (6 .. 26 here) and
 * drop_flags (SVO_IGNORE_* bits only). It is svo_voxel_map_bytes(log2_capacity) = 256 + 40 * capacity bytes of device
 * memory, 16-byte aligned: a header, and per entry
 *   key u64;  count, sx, sy, sz, sr, sg, sb, last u32          an empty entry: key = ~0, everything else 0
 * The header holds a magic word, the params and the counters of svo_voxel_map_info. A map is valid from its
 * svo_voxel_clear on; every other entry rejects a map whose header does not hold exactly the params it is given.
 *
 * Key of a record (x, y, z, color, flags). Per coordinate c, in float32, each operation rounded once:
 *   t = c / voxel;  q = floorf(t)
 * The record is OUTSIDE unless fabsf(q) < 1048576.0f holds for all three coordinates (so a NaN or an infinity is
 * outside). Otherwise
 *   i = (int)q + 1048576                       1 <= i < 2^21
 *   o = min(255u, (uint32_t)((t - q) * 256.0f))  the sub-voxel offset
 *   key = ix << 42 | iy << 21 | iz
 *
 * Skipped records. A record with flags & SVO_CLOUD_DROPPED or flags & drop_flags is never offered: it changes
 * nothing and counts nowhere.
 *
 * Fusing an offered record with stamp s (a u32 of the span it comes from). An outside record only counts in
 * n_outside. Otherwise the entry of its key is found or claimed (n_voxels += 1 when claimed) and
 *   count += 1;  sx += ox, sy += oy, sz += oz;  sr += color[0], sg += color[1], sb += color[2];  last = max(last, s)
 * and n_fused += 1. Every sum is modulo 2^32: a voxel is meaningful up to 2^32 / 255 = 16843009 records; a wrapped
 * sum is still the same in every run.
 *
 * Placement (a diagnostic fact, so that tests can craft probe chains; callers may not rely on where an entry lies):
 *   home = (key * 0x9E3779B97F4A7C15) >> (64 - log2_capacity)   (the product modulo 2^64)
 * and linear probing, step +1 modulo capacity.
 *
 * Load bound. A fuse is admitted only if, for every map it names,
 *   n_voxels + (records of all spans of this call into that map) <= capacity - capacity / 4
 * with n_voxels the header's. The check is on the bound (every record might claim an entry; skipped and outside
 * records count) and is made on the host before any launch: the rule of SVO_MAP_TOO_SMALL. A probe therefore always
 * ends and no record is lost to a full table; `overflow` counts records whose probe visited every entry, and stays 0.
 *
 * Extraction with a filter (min_count, min_stamp): an entry is kept iff count >= max(1, min_count) and
 * last >= min_stamp. The kept entries leave in ascending key order (lexicographic in ix, iy, iz), each as one
 * svo_map_point:
 *   x = (float)(((double)(ix - 1048576) + ((double)sx / (double)count + 0.5) / 256.0) * (double)voxel)
 * in double, each operation rounded once (no fused multiply-add), one rounding to float32; y, z alike;
 *   color[k] = min(255, (sum_k + count / 2) / count)  in 64-bit integers;  flags = 0.
 *
 * How it runs (voxel.hip): the fuse is one launch for many spans into many maps, one lane per record; the lanes of a
 * wavefront that hold the same key elect a leader, which alone probes (the claim is a 64-bit compare-and-swap of ~0)
 * and adds the group's sums. Probe and election loops are bounded (capacity and 64 rounds); nothing spins or waits.
 * The extraction counts, scans, writes (key, entry) pairs, sorts them by key and gathers. */
typedef struct svo_voxel_params {   /* 16 bytes */
    float    voxel;                 /* the voxel edge: finite, > 0                                          */
    int32_t  log2_capacity;         /* stage entries: 6 .. 26                                               */
    uint32_t drop_flags;            /* records with (flags & drop_flags) != 0 are skipped; SVO_IGNORE_* bits only */
    int32_t  _reserved;             /* 0                                                                    */
} svo_voxel_params;

typedef struct svo_voxel_map {      /* 24 bytes: a map and the params it was cleared with                   */
    void            *data;          /* device, 16-byte aligned, svo_voxel_map_bytes(params.log2_capacity)   */
    svo_voxel_params params;
} svo_voxel_map;

typedef struct svo_voxel_span {     /* 24 bytes */
    const svo_map_point *points;    /* device, 16-byte aligned (n = 0: not read)                            */
    int64_t  n;                     /* >= 0 records                                                         */
    int32_t  map;                   /* index into the call's maps                                           */
    uint32_t stamp;                 /* what `last` of the entries it reaches is raised to                   */
} svo_voxel_span;

typedef struct svo_voxel_map_info { /* 48 bytes */
    float    voxel;
    int32_t  log2_capacity;
    uint32_t drop_flags;
    int32_t  _pad;
    int64_t  n_voxels;              /* claimed entries                                                      */
    int64_t  n_fused;               /* records added to an entry                                            */
    int64_t  n_outside;             /* offered records that were outside                                    */
    int64_t  overflow;              /* records whose probe visited every entry (0: see the load bound)      */
} svo_voxel_map_info;

typedef struct svo_voxel_filter {   /* 16 bytes */
    uint32_t min_count;             /* kept: count >= max(1, min_count)                                     */
    uint32_t min_stamp;             /* kept: last >= min_stamp                                              */
    int32_t  _reserved[2];          /* 0                                                                    */
} svo_voxel_filter;

/* the bytes of a map, without a GPU; 0 for a log2_capacity outside 6 .. 26 */
int64_t svo_voxel_map_bytes(int log2_capacity);
/* Stage entries, complete on return. SVO_ERR_INVALID with nothing written: bad params (voxel not finite or <= 0,
 * log2_capacity outside 6 .. 26, drop_flags bits that are no SVO_IGNORE_* bit, _reserved != 0), a NULL or not 16-byte
 * aligned map or records, a negative n, a span that names no map of the call, a map named twice in one call, and (all
 * but svo_voxel_clear) a map that was not cleared with the same params.
 * svo_voxel_clear: every entry empty, the counters 0, the header holds the params. */
int svo_voxel_clear(svo_handle *h, void *map, const svo_voxel_params *params);
/* n_spans spans into n_maps maps in one launch (host arrays). SVO_ERR_CAPACITY with nothing written if the load bound
 * of any named map fails. */
int svo_voxel_fuse(svo_handle *h, int n_spans, const svo_voxel_span *spans, int n_maps, const svo_voxel_map *maps);
/* the params and counters the map's header holds */
int svo_voxel_info(svo_handle *h, const void *map, svo_voxel_map_info *info);
/* the kept entries as records points[0, *n_points) (device, 16-byte aligned); nothing else is written. filter == NULL
 * keeps every entry. points == NULL only counts. SVO_ERR_CAPACITY if the kept count exceeds `capacity`: *n_points is
 * set and nothing is written. The (key, entry) pairs and the sort's temporary storage live in the handle's
 * workspace: 24 bytes per kept entry and what the sort asks for. */
int svo_voxel_extract(svo_handle *h, const svo_voxel_map *map, const svo_voxel_filter *filter, svo_map_point *points,
                      int64_t capacity, int64_t *n_points);

/* Voxel maps inside a ctx: every slot can own one, and three queued jobs fuse the slots' dense clouds into them, read
 * them out and clear them.
 *
 * What a map is not. A map is an accumulator of the SLOT, not state of the sequence that runs in it: only fuse and
 * clear jobs change it. svo_ctx_restart_sequences, svo_submit_load, a trim, a rig assignment and the end of a
 * sequence leave it alone; snapshots do not carry it. A caller that wants a map per run clears it at the restart.
 *
 * svo_ctx_set_voxel_maps gives each named slot (seqs == NULL: every slot) a cleared map of its own with these params
 * (log2_capacity 10 .. 26), replacing one it had; params == NULL takes the maps away. It is a setter: it waits for the
 * queues, like svo_ctx_set_keyframe_window. A map's svo_voxel_map_bytes count in svo_memory.device_bytes; a ctx that
 * never sets maps allocates, launches and copies nothing more. svo_get_voxel_map_info waits too; SVO_ERR_INVALID for a
 * slot without a map. */
int svo_ctx_set_voxel_maps(svo_ctx *ctx, const int *seqs, int n, const svo_voxel_params *params);
int svo_get_voxel_map_info(svo_ctx *ctx, int seq, svo_voxel_map_info *info);

/* svo_submit_fuse_clouds is queued like a cloud job: it sees what was submitted before it and nothing after, only the
 * groups that own a named slot get work, and the slots' sequences are not changed. Per named slot it computes exactly
 * the records that svo_submit_export_cloud_checked(what, ..., style with layout = SVO_CLOUD_ORGANIZED and frame =
 * SVO_CLOUD_WORLD, check) delivers for that slot at that queue position (the same launches, in device mode, into a
 * block of the group; they never leave the device) and fuses them with `stamp` into the slot's map: one fuse launch
 * per chunk of slots (the chunk of "clouds", with 16 * points_per_slot more per slot; SVO_CLOUD_CHUNK_SLOTS lowers it).
 * info[i] belongs to seqs[i], is host memory and is valid at svo_wait:
 *   SVO_FUSE_OK      fused. n_offered: the cloud's kept count (its records without SVO_CLOUD_DROPPED); n_fused,
 *                    n_outside: what this job added to the map's counters; n_voxels: the map's entries afterwards
 *   SVO_FUSE_NONE    the cloud job would give SVO_CLOUD_NONE (no frame, or no keyframe): nothing is fused
 *   SVO_FUSE_NO_MAP  the slot has no map (this comes first)
 *   SVO_FUSE_FULL    n_voxels + points_per_slot > capacity - capacity / 4 (the load bound, on the bound, checked before
 *                    any launch with the ctx's host mirror of n_voxels): nothing is fused, the ctx does not fail. The
 *                    caller moves the map into a larger table (svo_ctx_resize_voxel_maps, "voxel entries").
 * The mirror of a map's counters is refreshed from the headers the job copies back anyway.
 * Rejected with SVO_ERR_INVALID and nothing queued: everything svo_submit_export_cloud_checked rejects of what, seqs,
 * style and check; style->frame != SVO_CLOUD_WORLD; style->layout != 0; a NULL info.
 * Memory, per group, made by the first fuse job and replaced when outgrown (svo_memory.device_bytes): the records of
 * a chunk, 16 * points_per_slot per slot, and the chunk's tables (up256(24 m) + up256(64 m) + up256(32 m) bytes for m
 * slots, device and pinned), beside the cloud job's own blocks. */
enum { SVO_FUSE_OK = 0, SVO_FUSE_NONE = 1, SVO_FUSE_NO_MAP = 2, SVO_FUSE_FULL = 3 };

typedef struct svo_fuse_info {      /* 64 bytes, host, one per named slot */
    int32_t seq, run;               /* slot and ordinal of its run                                          */
    int32_t frame_id;               /* of the slot's current frame; -1: empty slot                          */
    int32_t keyframe_id;            /* LAST_KEYFRAMES: the keyframe used (-1: none); FRAMES: -1             */
    int32_t status;                 /* SVO_FUSE_*                                                           */
    int32_t n_offered;              /* the cloud's kept count                                               */
    int32_t n_fused, n_outside;     /* added by this job                                                    */
    int64_t n_voxels;               /* of the map after the job (NO_MAP: 0)                                 */
    float   pose[6];                /* the pose used, as svo_cloud_segment.pose                             */
} svo_fuse_info;

int svo_submit_fuse_clouds(svo_ctx *ctx, int what, const int *seqs, int n, const svo_cloud_style *style,
                           const svo_stereo_check *check, uint32_t stamp, svo_fuse_info *info);
int svo_fuse_clouds(svo_ctx *ctx, int what, const int *seqs, int n, const svo_cloud_style *style,
                    const svo_stereo_check *check, uint32_t stamp, svo_fuse_info *info);   /* submit + wait */

/* svo_submit_export_voxel_maps follows svo_submit_export_map: a region per named slot, a shared filter, a 64-byte
 * segment per slot in host memory, records in host or device memory (mem). A slot's entries are kept iff
 * count >= max(1, filter->min_count) and last >= max(filter->min_stamp, region.min_stamp), and leave in key order into
 * points[first_point, first_point + n_points): exactly those records are written. A slot whose n_voxels (the host
 * mirror: the bound, checked before any launch) exceeds its point_capacity comes back SVO_VOXEL_TOO_SMALL with
 * n_voxels the capacity needed and nothing else written; a slot without a map SVO_VOXEL_NO_MAP. Host mode stages the
 * records in a block of the group and copies the kept prefix out. Rejected with SVO_ERR_INVALID: a bad mem, a slot
 * out of range or named twice, a negative region field or a non-zero _reserved, points not 16-byte aligned, a region
 * with a capacity and NULL points. Memory (svo_memory.device_bytes), per group: 4 bytes per tile of 256 entries of the
 * largest map, 24 bytes per kept entry and what the sort asks for, and in host mode 16 bytes per kept entry. */
enum { SVO_VOXEL_OK = 0, SVO_VOXEL_NO_MAP = 1, SVO_VOXEL_TOO_SMALL = 2 };

typedef struct svo_voxel_region {   /* 32 bytes */
    int64_t  first_point;           /* the slot's records start at dst->points[first_point]                 */
    int64_t  point_capacity;        /* records the region holds                                             */
    uint32_t min_stamp;             /* this slot's entries with last < min_stamp are not kept               */
    int32_t  _reserved[3];          /* 0                                                                    */
} svo_voxel_region;

typedef struct svo_voxel_segment {  /* 64 bytes, host, one per named slot */
    int32_t seq, run;
    int32_t frame_id;
    int32_t status;                 /* SVO_VOXEL_*                                                          */
    int64_t first_point;            /* the region's                                                         */
    int64_t n_points;               /* records written (0 unless SVO_VOXEL_OK)                              */
    int64_t n_voxels;               /* the map's entries: the point_capacity that is always enough          */
    int64_t n_fused;                /* the map's counter                                                    */
    float   voxel;
    int32_t log2_capacity;
    int64_t _pad;
} svo_voxel_segment;

typedef struct svo_voxel_dst {
    svo_voxel_segment *segments;    /* HOST memory always, >= n entries                                     */
    svo_map_point     *points;      /* host or device (mem), 16-byte aligned; NULL: every point_capacity is 0 */
} svo_voxel_dst;

int svo_submit_export_voxel_maps(svo_ctx *ctx, const int *seqs, int n, const svo_voxel_region *regions,
                                 const svo_voxel_filter *filter, const svo_voxel_dst *dst, int mem);
int svo_export_voxel_maps(svo_ctx *ctx, const int *seqs, int n, const svo_voxel_region *regions,
                          const svo_voxel_filter *filter, const svo_voxel_dst *dst, int mem);   /* submit + wait */
/* queued: the maps of the named slots become empty (a slot without a map is skipped) */
int svo_submit_clear_voxel_maps(svo_ctx *ctx, const int *seqs, int n);

/* ---- voxel prune: a voxel map reduced in place to the entries a keep rule names ------------
 * A map of "voxel maps" only grows. A prune gives entries back without a trip through the host: the map follows the
 * camera (a box around a centre), forgets what was not seen lately (`last`) and sheds entries that never gathered
 * evidence (`count`), so that a fused map can run without end.
 *
 * The keep rule (svo_voxel_keep). Centre voxel: per coordinate, ci is the index i that the key rule of "voxel maps"
 * gives center (t = c / voxel; q = floorf(t); i = (int)q + 1048576, in float32); a centre that the key rule calls
 * outside (a NaN and an infinity too) is rejected. An entry with key parts (ix, iy, iz) is INSIDE THE BOX iff
 *   |ix - cix| <= radius && |iy - ciy| <= radius && |iz - ciz| <= radius
 * in integers (a Chebyshev box of 2 radius + 1 voxels per axis: membership is exact). radius < 0: there is no box and
 * center is not read. An entry is KEPT iff count >= max(1, min_count) and last >= min_stamp and, with radius >= 0,
 * it is inside the box.
 *
 * After a prune the map holds exactly the kept entries, each with its eight accumulators unchanged, and n_voxels is
 * the kept count. n_fused, n_outside and overflow keep their values: they are cumulative over the map's life (from
 * its last clear), not a description of the entries it holds now. Placement follows the rule of "voxel maps" (home by
 * the multiplicative hash, linear probing): every kept entry is reachable from its home without crossing an empty
 * entry, so a later fuse of a record with a kept key finds the entry and claims no second one. Where an entry lies
 * stays a diagnostic fact: a prune may move kept entries.
 *
 * What follows, and what the tests hold:
 *   - an extraction after prune(K) with filter F equals, byte for byte, an extraction before it with "F and K";
 *   - prune(K) twice equals prune(K) once;
 *   - a prune that removes nothing writes no byte of the map;
 *   - a prune that keeps nothing leaves what svo_voxel_clear leaves, but for the three cumulative counters;
 *   - fusing further spans after a prune gives what the statement gives from the pruned content;
 *   - the load bound of the next fuse uses the new n_voxels.
 *
 * How it runs (voxel.hip): blanking keys would cut the probe chains behind them, so the map is rebuilt in place:
 * count and scan with the keep rule, the kept entries (40 bytes each) to a staging block, the table cleared (the
 * header stays), one lane per staged entry reinserts (the fuse's probe and claim, bounded by the capacity), and
 * n_voxels is set. Six launches ordered by the stream; nothing spins or waits for another workgroup, and nothing is
 * read back in between: each rebuild kernel compares the scan's total with the header's n_voxels and returns at once
 * when they are equal. */
typedef struct svo_voxel_keep {     /* 32 bytes */
    uint32_t min_count;             /* kept: count >= max(1, min_count)                                     */
    uint32_t min_stamp;             /* kept: last >= min_stamp                                              */
    float    center[3];             /* the box's centre, in the map's coordinates                           */
    int32_t  radius;                /* in voxels; < 0: no box (center is not read)                          */
    int32_t  _reserved[2];          /* 0                                                                    */
} svo_voxel_keep;

typedef struct svo_voxel_prune_result { /* 32 bytes */
    int64_t n_before;               /* the map's n_voxels before the prune                                  */
    int64_t n_kept;                 /* and after it                                                         */
    int32_t center_voxel[3];        /* (cix, ciy, ciz); radius < 0: 0                                       */
    int32_t _pad;
} svo_voxel_prune_result;

/* Stage entry, complete on return; `out` may be NULL. The staging block lives in the handle's workspace:
 * up256(40 * n_voxels) bytes, sized on the header's n_voxels (the bound of what is kept: no count is read back before
 * the launches), beside the tile offsets (4 bytes per tile of 256 entries). SVO_ERR_CAPACITY with nothing written if
 * that block would exceed 1 GiB. SVO_ERR_INVALID with nothing written: what svo_voxel_extract rejects of the map, a
 * NULL keep, a non-zero _reserved and, with radius >= 0, a centre that is not finite or lies outside by the key rule. */
int svo_voxel_prune(svo_handle *h, const svo_voxel_map *map, const svo_voxel_keep *keep, svo_voxel_prune_result *out);

/* svo_submit_prune_voxel_maps prunes the maps of the named slots inside a ctx. It is queued like a fuse job: it sees
 * what was submitted before it and nothing after, only the groups that own a named slot get work, no other group is
 * drained and the slots' sequences are not changed. keep's min_count, min_stamp and radius hold for every named slot;
 * the centre of slot seqs[i] (not read with radius < 0) comes by center_mode:
 *   SVO_PRUNE_CENTER_GIVEN  centers[3 i .. 3 i + 2] (host, copied at the call); centers == NULL: keep->center for all.
 *                           Checked at the call against the voxel edge of the slot's map as the ctx knows it then.
 *   SVO_PRUNE_CENTER_POSE   the slot's camera centre at that queue position: the world-frame point that the cloud
 *                           job's camera-to-world transform (w = R loc + t of the slot's current pose, "clouds") gives
 *                           the camera-frame origin, which is the pose's translation pose[0 .. 2]. It is taken by the
 *                           group's worker when the job runs, so a map that follows the camera needs no wait.
 * info[i] belongs to seqs[i], is host memory and is valid at svo_wait:
 *   SVO_PRUNE_OK         pruned: n_before and n_kept are the map's n_voxels before and after, center and center_voxel
 *                        the centre used and its voxel (radius < 0: 0)
 *   SVO_PRUNE_NO_MAP     the slot has no map (this comes first)
 *   SVO_PRUNE_NO_POSE    pose mode on an empty slot (no frame yet), or with a camera centre that is not finite or
 *                        lies outside by the key rule: nothing is pruned
 *   SVO_PRUNE_TOO_LARGE  staging the map's n_voxels entries would exceed 1 GiB (svo_voxel_prune's bound, with the ctx's
 *                        host mirror of n_voxels): the map is unchanged and the ctx does not fail
 * The job copies the headers back and refreshes the ctx's mirror of the maps' counters in queue order: a fuse job
 * queued behind a prune job settles its SVO_FUSE_FULL on the pruned count, with no wait between them.
 * Rejected with SVO_ERR_INVALID and nothing queued: a NULL keep or info, a non-zero _reserved, a center_mode that is
 * neither, a slot out of range or named twice and, in given mode with radius >= 0, a centre that is not finite or
 * lies outside by the key rule for its slot's map.
 * Memory, per group, made by the first prune job and replaced when outgrown (svo_memory.device_bytes): one block of
 *   up256(4 * (capacity / 256 + 1)) + up256(40 * n_voxels)
 * bytes (capacity / 256 at least 1), the largest that a slot of a job has needed: the tile offsets and the staging. */
enum { SVO_PRUNE_OK = 0, SVO_PRUNE_NO_MAP = 1, SVO_PRUNE_NO_POSE = 2, SVO_PRUNE_TOO_LARGE = 3 };
enum { SVO_PRUNE_CENTER_GIVEN = 0, SVO_PRUNE_CENTER_POSE = 1 };

typedef struct svo_prune_info {     /* 64 bytes, host, one per named slot */
    int32_t seq, run;               /* slot and ordinal of its run                                          */
    int32_t frame_id;               /* of the slot's current frame; -1: empty slot                          */
    int32_t status;                 /* SVO_PRUNE_*                                                          */
    int64_t n_before;               /* the map's n_voxels before the job (NO_MAP: 0)                        */
    int64_t n_kept;                 /* and after it (not pruned: n_before)                                  */
    float   center[3];              /* the centre used (radius < 0, NO_MAP, NO_POSE on an empty slot: 0)    */
    int32_t center_voxel[3];        /* its voxel by the key rule (not OK: 0)                                */
    int32_t _pad[2];
} svo_prune_info;

int svo_submit_prune_voxel_maps(svo_ctx *ctx, const int *seqs, int n, const svo_voxel_keep *keep, int center_mode,
                                const float *centers, svo_prune_info *info);
int svo_prune_voxel_maps(svo_ctx *ctx, const int *seqs, int n, const svo_voxel_keep *keep, int center_mode,
                         const float *centers, svo_prune_info *info);   /* submit + wait */

/* ---- sgm fusion: voxel maps fed by the clouds of SGM maps ------------
 * A voxel map averages whatever depth it is given, and it lives for the whole run; the winner-takes-all disparities of
 * "dense" are whole numbers, so z = baseline / d is a stack of sheets. This section and the two after it give the
 * three consumers of a slot's dense cloud inside the ctx (the fuse job, the scene job's live layer, the occluded AR
 * job) an SGM form. None has new arithmetic, a new kernel or a new kind of queue entry: each is the consumer's own
 * statement with svo_submit_export_cloud_sgm(what, ..., style, sgm, check, ...) in the place of
 * svo_submit_export_cloud_checked(what, ..., style, check, ...): the same records bit for bit, at the same queue
 * position, into the same block that never leaves the device, and then the consumer's launches as they are.
 *
 * svo_submit_fuse_clouds_sgm is svo_submit_fuse_clouds with the params. `check` is the check of "sgm cross-check" (the
 * second SGM map of the mirrored pair, not the reverse search of "cross-check"); NULL or lr == 0: unchecked.
 * sgm == NULL IS svo_submit_fuse_clouds: the same launches, bytes, memory and rejections. Statuses and svo_fuse_info
 * are unchanged; SVO_FUSE_FULL is settled as before, ahead of any launch. max_mean_cost bounds the aggregated cost
 * over four paths, as in "sgm cross-check".
 * Rejected with SVO_ERR_INVALID and nothing queued: everything svo_submit_fuse_clouds rejects and everything
 * svo_submit_export_cloud_sgm rejects of style, sgm and check: a bad param (paths != 4 among them), the 16-bit bound,
 * an effective search_x > 63, a non-zero _reserved, a check that is on with max_lr_diff <= 0.
 * Memory, per group: the records and tables of svo_submit_fuse_clouds and the cloud job's staging block (slot_bytes of
 * "clouds" per slot of a chunk), no reverse block whatever the check; the SGM planes of a chunk's delivered slots go
 * through the group's block of "sgm" under its rule (slot_bytes of "sgm cross-check", chunks of max(1, 512 MiB /
 * slot_bytes), SVO_SGM_CHUNK_SLOTS, one slot always fits), counted in svo_memory.device_bytes. The chunk of the fuse
 * job is max(1, 256 MiB / (slot_bytes of "clouds" + 16 * points_per_slot)). A job without sgm, and a ctx that never
 * asks, allocate, launch and copy what they did.
 * No stage entry: the stage form is svo_cloud_points_sgm followed by svo_voxel_fuse. */
int svo_submit_fuse_clouds_sgm(svo_ctx *ctx, int what, const int *seqs, int n, const svo_cloud_style *style,
                               const svo_sgm_params *sgm, const svo_stereo_check *check, uint32_t stamp,
                               svo_fuse_info *info);
int svo_fuse_clouds_sgm(svo_ctx *ctx, int what, const int *seqs, int n, const svo_cloud_style *style,
                        const svo_sgm_params *sgm, const svo_stereo_check *check, uint32_t stamp,
                        svo_fuse_info *info);   /* submit + wait */

/* ---- sgm scene clouds: the scene picture's live layer from SGM maps ------------
 * svo_submit_export_scenes_clouds_sgm is svo_submit_export_scenes_clouds with the params: with live == 1 the live
 * layer of named slot i is exactly the records svo_submit_export_cloud_sgm(clouds->what, ..., clouds->cloud in the
 * organized layout, sgm, &clouds->check, ...) delivers for that slot at that queue position. clouds->check is then the
 * check of "sgm cross-check"; lr == 0: unchecked. Segments, svo_scene_cloud_info, the extra spans, the splat pass
 * and the tile render are unchanged. sgm == NULL IS svo_submit_export_scenes_clouds. A non-NULL sgm is validated
 * whatever clouds says (also with clouds == NULL or live == 0, where the job is otherwise the plain one and the
 * params are not used).
 * Rejected with SVO_ERR_INVALID and nothing queued: everything svo_submit_export_scenes_clouds rejects, a bad sgm, and
 * with live == 1 everything svo_submit_export_cloud_sgm rejects of clouds->cloud, sgm and clouds->check (as listed
 * under "sgm fusion").
 * Memory, per group: the blocks of "scene clouds" with
 *   chunk = max(1, 256 MiB / (key_bytes + [live: slot_bytes + 16 * points_per_slot]))
 * (no reverse_bytes term, and no reverse block), and the SGM planes of a chunk's delivered slots in the group's block of
 * "sgm" under its rule, as in "sgm fusion". Per chunk the order on the group's stream is: cost volumes, paths, check,
 * cloud write, clear, splat, tile render. A job without sgm allocates, launches and copies what it did.
 * No stage entry: the stage form is svo_cloud_points_sgm followed by svo_render_scene_clouds. */
int svo_submit_export_scenes_clouds_sgm(svo_ctx *ctx, const int *seqs, int n, const svo_scene_style *style,
                                        const svo_scene_clouds *clouds, const svo_sgm_params *sgm,
                                        const svo_scene_camera *cameras, const svo_scene_dst *dst, int mem);
int svo_export_scenes_clouds_sgm(svo_ctx *ctx, const int *seqs, int n, const svo_scene_style *style,
                                 const svo_scene_clouds *clouds, const svo_sgm_params *sgm,
                                 const svo_scene_camera *cameras, const svo_scene_dst *dst, int mem);   /* submit + wait */

/* ---- sgm ar occlusion: meshes hidden behind the depth of SGM maps ------------
 * svo_submit_export_ar_occluded_sgm is svo_submit_export_ar_occluded with the params: with on == 1 the occluder of
 * named slot i is exactly the records svo_submit_export_cloud_sgm(SVO_EXPORT_FRAMES, ..., occlusion->cloud in the
 * camera frame and the organized layout, sgm, &occlusion->check, ...) delivers for that slot at that queue position.
 * occlusion->check is then the check of "sgm cross-check"; lr == 0: unchecked. The pixel rule, the pictures' layout,
 * segments and svo_ar_visibility are unchanged. sgm == NULL IS svo_submit_export_ar_occluded. A non-NULL sgm is
 * validated whatever occlusion->on says, like the occlusion's scalar fields; with occlusion == NULL or on == 0 the job
 * is otherwise svo_submit_export_ar and the params are not used.
 * Rejected with SVO_ERR_INVALID and nothing queued: everything svo_submit_export_ar_occluded rejects, a bad sgm, and
 * with on == 1 everything svo_submit_export_cloud_sgm rejects of occlusion->cloud, sgm and occlusion->check (as listed
 * under "sgm fusion").
 * Memory, per group: the blocks of "ar occlusion" with
 *   chunk = max(1, 256 MiB / (slot_bytes + 16 * points_per_slot))
 * (no reverse_bytes term, and no reverse block), and the SGM planes of a chunk's delivered slots in the group's block of
 * "sgm" under its rule, as in "sgm fusion". Per chunk the order on the group's stream is: cost volumes, paths, check,
 * cloud write, set-up, tile render. A job without sgm allocates, launches and copies what it did.
 * No stage entry: the stage form is svo_cloud_points_sgm followed by svo_render_ar_occluded. */
int svo_submit_export_ar_occluded_sgm(svo_ctx *ctx, const int *seqs, int n, const svo_ar_style *style,
                                      const svo_ar_occlusion *occlusion, const svo_sgm_params *sgm,
                                      const svo_ar_mesh *meshes, int n_meshes, const svo_ar_instance *instances,
                                      const int *first, int n_instances, const svo_ar_dst *dst, int mem);
int svo_export_ar_occluded_sgm(svo_ctx *ctx, const int *seqs, int n, const svo_ar_style *style,
                               const svo_ar_occlusion *occlusion, const svo_sgm_params *sgm,
                               const svo_ar_mesh *meshes, int n_meshes, const svo_ar_instance *instances,
                               const int *first, int n_instances, const svo_ar_dst *dst, int mem);   /* submit + wait */

/* ---- voxel carve: entries of a voxel map removed where the current frame's dense depth sees through them ------------
 * A voxel map averages whatever it is given for the whole run, and "voxel prune" forgets entries by count, stamp and a
 * box. Neither removes an entry that the camera now sees to be wrong: a wrong disparity that survived its check and
 * claimed a voxel in front of the wall, or the ghost of an object that has moved. A carve removes the entries that lie
 * in FRONT of what the camera measures along their ray: the occluder of "ar occlusion" (the organized, camera-frame cloud
 * of the very frame the camera shows) read the other way round.
 *
 * Inputs: a map (svo_voxel_map), a camera (svo_ar_camera), the image size W x H, an occluder (svo_ar_occluder: records,
 * cols, rows, step) and a svo_voxel_carve_rule. Per non-empty entry; all arithmetic float32, each operation rounded once,
 * without contraction, but for step 1:
 *   1 point     w = the point the entry extracts to by the formula of "voxel maps": per coordinate computed in double and
 *               rounded once to float. An entry with last > max_last is no candidate: it is kept.
 *   2 camera    c_k = ((V[4k] * w_0 + V[4k+1] * w_1) + V[4k+2] * w_2) + V[4k+3], the c_k of "ar". Any c_k not finite, or
 *               c_2 < near: the entry is kept.
 *   3 pixel     u = (fx * c_0) / c_2 + cx, v = (fy * c_1) / c_2 + cy. The entry is kept unless
 *               u >= 0.0f && u < (float)W && v >= 0.0f && v < (float)H (a NaN keeps it). px = (int)u, py = (int)v; the
 *               cell is ix = px / step, iy = py / step.
 *   4 evidence  a cell HAS AN OCCLUDER DEPTH zo by the rule of "ar occlusion", with this struct's drop_flags. ring = 0:
 *               the evidence is the cell's zo. ring = 1: zmin = the minimum of zo over the cells (ix + dx, iy + dy), dx,
 *               dy in {-1, 0, 1}, that lie inside the lattice. If the cell itself lies outside the lattice (ix >= cols
 *               or iy >= rows), or any cell consulted has no occluder depth, or records == NULL, the evidence is
 *               incomplete: the entry is kept. The ring keeps the rim of a foreground object from being carved by a
 *               background cell beside it when step > 1.
 *   5 verdict   the entry is CARVED iff c_2 + margin < zmin: one add, one comparison. The camera measured a surface more
 *               than margin behind the entry.
 * One contradiction removes an entry (no votes: that would need a ninth accumulator); ring, margin and max_last are
 * the guards.
 *
 * With an optional svo_voxel_keep an entry STAYS iff the keep rule of "voxel prune" keeps it and it is not carved
 * (keep == NULL: every entry is kept by the keep rule). The map is rebuilt exactly as a prune rebuilds it: the same
 * placement guarantees, the eight accumulators unchanged, n_voxels = the entries that stay, the three cumulative
 * counters untouched, and a call that removes nothing writes no byte of the map.
 *
 * Result, exact integers summed on the device (one 64-bit atomic add per count and workgroup after a reduction inside
 * it, so arrival order cannot matter): n_before, n_kept = the map's n_voxels before and after; n_tested = the entries
 * that reached step 5; n_carved = those step 5 carves, whether or not the keep rule rejects them too.
 *
 * How it runs (voxel.hip): the prune's six launches with its count and stage kernels instantiated on the joined rule.
 * The carve is evaluated once, in the count pass, which leaves one 64-bit ballot word per wavefront in the workspace;
 * the stage pass reads the words. */
typedef struct svo_voxel_carve_rule {    /* 32 bytes */
    float    margin;                /* finite, >= 0, in the unit of the depths                              */
    float    near;                  /* finite, > 0                                                          */
    uint32_t max_last;              /* an entry with last > max_last is kept                                */
    uint32_t drop_flags;            /* occluder records with any of these flag bits give no depth           */
    int32_t  ring;                  /* 0: the entry's cell; 1: the cell and its neighbours                  */
    int32_t  _reserved[3];          /* 0                                                                    */
} svo_voxel_carve_rule;

typedef struct svo_voxel_carve_result { /* 32 bytes */
    int64_t n_before;               /* the map's n_voxels before the call                                   */
    int64_t n_kept;                 /* and after it                                                         */
    int64_t n_tested;               /* entries that reached step 5                                          */
    int64_t n_carved;               /* entries that step 5 carves                                           */
} svo_voxel_carve_result;

/* Stage entry, complete on return; keep and result may be NULL. The workspace is svo_voxel_prune's (the tile offsets and
 * the staging block, with its 1 GiB bound and SVO_ERR_CAPACITY), followed by the ballot words (8 bytes per 64 entries)
 * and the counters. SVO_ERR_INVALID with nothing written: what svo_voxel_prune rejects of the map and of a non-NULL
 * keep; what svo_render_ar_occluded rejects of a camera and an occluder (a NULL pointer to either too); a NULL carve, a
 * margin that is negative or not finite, a near that is not finite or <= 0, a ring that is neither 0 nor 1, a non-zero
 * _reserved; width or height outside 1 .. 32768. An occluder with records == NULL gives no evidence anywhere: the call
 * is a plain prune by keep and n_tested = n_carved = 0. */
int svo_voxel_carve(svo_handle *h, const svo_voxel_map *map, const svo_ar_camera *camera, int width, int height,
                    const svo_ar_occluder *occluder, const svo_voxel_carve_rule *carve, const svo_voxel_keep *keep,
                    svo_voxel_carve_result *result);

/* svo_submit_carve_voxel_maps carves the maps of the named slots inside a ctx with the frame each slot holds at that
 * queue position. It is queued like a prune job and is no new kind of queue entry: it is the prune entry carrying a
 * carve, as the SGM jobs carry their params. keep (NULL: every entry is kept by the keep rule), center_mode and centers
 * are the prune job's. Per named slot:
 *   occluder   exactly the records that svo_submit_export_ar_occluded would use at that queue position with `cloud` and
 *              `check`, or svo_submit_export_ar_occluded_sgm with `sgm`: the current frame, frame = SVO_CLOUD_CAMERA,
 *              organized, cols = W / step, rows = H / step, computed by the cloud job's own launches into the occluded AR
 *              job's block of the group; they never leave the device
 *   camera     svo_ar_camera_of_pose of the slot's current pose and rig (its deferred pose-filter update is flushed
 *              first, as for the AR job); the image size is the ctx's W x H
 * info[i] belongs to seqs[i], is host memory and is valid at svo_wait:
 *   SVO_CARVE_OK         carved: the four counts of svo_voxel_carve_result, and the pose the camera was made of
 *   SVO_CARVE_NO_MAP     the slot has no map (this comes first)
 *   SVO_CARVE_NONE       an empty slot (no frame yet, as SVO_CLOUD_NONE): nothing changes
 *   SVO_CARVE_NO_POSE, SVO_CARVE_TOO_LARGE   as SVO_PRUNE_NO_POSE and SVO_PRUNE_TOO_LARGE: nothing changes
 * The ctx's mirror of the maps' counters is refreshed in queue order: a fuse job queued behind a carve is admitted on
 * the carved count. Rejected with SVO_ERR_INVALID and nothing queued: everything svo_submit_export_ar_occluded(_sgm)
 * rejects of cloud, sgm and check (cloud.frame != SVO_CLOUD_CAMERA and cloud.layout != 0 too), everything
 * svo_submit_prune_voxel_maps rejects (of a non-NULL keep), everything svo_voxel_carve rejects of the carve, a NULL info.
 * Memory, per group, made on first use: the occluded AR job's cloud blocks and the prune job's block, which here also
 * holds the ballot words of the largest map and 256 bytes of counters per carved slot. A ctx that never carves
 * allocates, launches and copies nothing more; a prune job launches what it launched before. */
enum { SVO_CARVE_OK = 0, SVO_CARVE_NO_MAP = 1, SVO_CARVE_NO_POSE = 2, SVO_CARVE_TOO_LARGE = 3, SVO_CARVE_NONE = 4 };

typedef struct svo_carve_info {     /* 64 bytes, host, one per named slot */
    int32_t seq, run;               /* slot and ordinal of its run                                          */
    int32_t frame_id;               /* of the slot's current frame; -1: empty slot                          */
    int32_t status;                 /* SVO_CARVE_*                                                          */
    int64_t n_before;               /* the map's n_voxels before the job (NO_MAP: 0)                        */
    int64_t n_kept;                 /* and after it (not carved: n_before)                                  */
    int32_t n_tested, n_carved;     /* the stage result's counts; a map has at most 1 << 26 entries      */
    float   pose[6];                /* svo_get_pose at that queue position                                  */
} svo_carve_info;

int svo_submit_carve_voxel_maps(svo_ctx *ctx, const int *seqs, int n, const svo_cloud_style *cloud, const svo_sgm_params *sgm,
                                const svo_stereo_check *check, const svo_voxel_carve_rule *carve, const svo_voxel_keep *keep,
                                int center_mode, const float *centers, svo_carve_info *info);
int svo_carve_voxel_maps(svo_ctx *ctx, const int *seqs, int n, const svo_cloud_style *cloud, const svo_sgm_params *sgm,
                         const svo_stereo_check *check, const svo_voxel_carve_rule *carve, const svo_voxel_keep *keep,
                         int center_mode, const float *centers, svo_carve_info *info);   /* submit + wait */

/* ---- voxel entries: the raw entries of a voxel map packed out, merged in, moved to a table of another size ------------
 * An entry of "voxel maps" is a key and eight integer accumulators that only ever take commutative updates (add modulo
 * 2^32, max), so the accumulators are a complete, exact and order-free description of everything that was fused.
 * svo_voxel_extract gives the means and throws the counts, the sums and the stamps away; re-fusing the means gives
 * every voxel count 1. Here the entries themselves leave and enter a map: merging two maps entry by entry gives, to
 * the bit, the map that fusing the union of their records would have given, so a map can be saved, loaded, joined
 * with another and moved into a larger or smaller table without losing anything.
 *
 * Record. svo_voxel_entry: 40 bytes, 8-byte aligned: the key and acc[8] = count, sx, sy, sz, sr, sg, sb, last, exactly
 * the key and the accumulators of "voxel maps".
 *
 * Pack. A map and a svo_voxel_filter, by the kept rule of the extraction: count >= max(1, min_count) and
 * last >= min_stamp. The kept entries leave in ascending key order, each as one record with its eight accumulators
 * verbatim. Keys are unique, so the bytes are the same in every run, wherever the entries lay in their probe chains.
 *
 * Merge. A span of n records is offered to a map. A record is SKIPPED if bit 63 of its key is set (the empty key ~0
 * is one such), or its count is 0: it counts in n_skipped and nowhere else. Otherwise the entry of its key is found
 * or claimed (n_voxels += 1 when claimed) and, with ' for the record's values,
 *   count += count';  sx += sx', sy += sy', sz += sz', sr += sr', sg += sg', sb += sb'  (modulo 2^32);
 *   last = max(last, last')
 * and the header's n_fused += count' (a 64-bit sum); n_outside and overflow are untouched (overflow counts, as for a
 * fuse, records whose probe visited every entry, and the load bound keeps it 0). Keys may repeat inside a span and
 * across the spans of a call: the result is the same as if every underlying record had been fused.
 *
 * Voxel edge. A span carries the voxel edge its keys were made with. It must equal the map's `voxel` bit for bit,
 * otherwise the call is SVO_ERR_INVALID and nothing is written. Re-voxelising is not exact and is not offered.
 *
 * Load bound: that of the fuse, on the bound, checked on the host before any launch:
 *   n_voxels + (records of all spans of the call into that map) <= capacity - capacity / 4
 * (skipped records count). On failure the call is SVO_ERR_CAPACITY with nothing written.
 *
 * Rehash (resize). The entries of one map go into a cleared map with another log2_capacity and the same voxel and
 * drop_flags. Afterwards the new map holds exactly the old entries with their accumulators, the old n_voxels and the
 * three cumulative counters (n_fused, n_outside, overflow) of the old header. Placement follows the rule of "voxel
 * maps" (home by the new capacity, linear probing), so a fuse that follows finds every entry. The rehash is admitted
 * only if n_voxels <= capacity' - capacity' / 4. The old map is only read.
 *
 * How it runs (voxel.hip): the pack is the extraction's count, scan, pairs and sort with another gather (one lane per
 * kept entry, two 16-byte loads, one 40-byte record). The merge is one launch for many spans into many maps, cut into
 * tiles of 256 records like the fuse, one lane per record: the probe from the key's home, the claim by a 64-bit
 * compare-and-swap of ~0, then eight integer atomics, always atomics (another lane with the same key may find a
 * claimed key before the claimer's first add). The rehash is one lane per entry of the old table with the prune's
 * reinsert (keys are unique and the new table is private until the call returns: plain stores), and a one-lane launch
 * that copies the counters. Probe loops are bounded by the capacity; nothing spins or waits. */
typedef struct svo_voxel_entry {    /* 40 bytes */
    uint64_t key;                   /* ix << 42 | iy << 21 | iz                                             */
    uint32_t acc[8];                /* count, sx, sy, sz, sr, sg, sb, last                                  */
} svo_voxel_entry;

typedef struct svo_voxel_entry_span {   /* 24 bytes */
    const svo_voxel_entry *entries; /* device, 8-byte aligned (n = 0: not read)                             */
    int64_t  n;                     /* >= 0 records                                                         */
    int32_t  map;                   /* index into the call's maps                                           */
    float    voxel;                 /* the voxel edge the keys were made with: the map's, bit for bit       */
} svo_voxel_entry_span;

typedef struct svo_voxel_merge_result { /* 32 bytes, one per map of the call; exact integers summed on the device */
    int64_t n_offered;              /* records of the call's spans into this map                            */
    int64_t n_merged;               /* of them added to an entry                                            */
    int64_t n_skipped;              /* of them skipped                                                      */
    int64_t n_claimed;              /* entries claimed: what n_voxels grew by                               */
} svo_voxel_merge_result;

/* Stage entries, complete on return.
 * svo_voxel_pack follows svo_voxel_extract exactly: entries[0, *n) (device, 8-byte aligned) receive the kept entries
 * and nothing else is written; filter == NULL keeps every entry; entries == NULL only counts; SVO_ERR_CAPACITY if the
 * kept count exceeds `capacity`: *n is set and nothing is written. It rejects what svo_voxel_extract rejects, and the
 * workspace is the extraction's. */
int svo_voxel_pack(svo_handle *h, const svo_voxel_map *map, const svo_voxel_filter *filter, svo_voxel_entry *entries,
                   int64_t capacity, int64_t *n);
/* n_spans spans into n_maps maps in one launch (host arrays). SVO_ERR_INVALID with nothing written: what
 * svo_voxel_fuse rejects (entries need 8-byte alignment only), and a span whose voxel is not its map's bit for bit.
 * SVO_ERR_CAPACITY with nothing written if the load bound of any named map fails. results: n_maps records, host
 * memory, may be NULL. */
int svo_voxel_merge(svo_handle *h, int n_spans, const svo_voxel_entry_span *spans, int n_maps, const svo_voxel_map *maps,
                    svo_voxel_merge_result *results);
/* dst (device, 16-byte aligned, svo_voxel_map_bytes(dst_log2_capacity) bytes, need not be cleared) becomes the map of
 * src's entries with params (src's voxel, dst_log2_capacity, src's drop_flags). SVO_ERR_INVALID with nothing written:
 * what svo_voxel_extract rejects of src, a dst that is NULL, not 16-byte aligned or overlaps src's bytes (dst ==
 * src->data among them), a dst_log2_capacity outside 6 .. 26. SVO_ERR_CAPACITY by the admission rule: dst is then
 * untouched. */
int svo_voxel_rehash(svo_handle *h, const svo_voxel_map *src, void *dst, int dst_log2_capacity);

/* Voxel entries inside a ctx: the maps of the slots saved, loaded and resized. svo_submit_save, svo_submit_load and
 * snapshots still leave maps alone ("What a map is not"): a map travels by the three entries below.
 *
 * svo_submit_save_voxel_maps is svo_submit_export_voxel_maps with svo_voxel_entry records in place of points: the
 * same svo_voxel_region per named slot (first_point and point_capacity count entry records), the same shared filter
 * and region.min_stamp, the same 64-byte svo_voxel_segment per slot in host memory (n_points counts entries), the
 * same statuses SVO_VOXEL_OK / NO_MAP / TOO_SMALL decided on the mirror before any launch, records in host or device
 * memory (mem): exactly entries[first_point, first_point + n_points) are written, in key order. It is queued behind
 * what was submitted so far and only the groups that own a named slot get work. Rejected with SVO_ERR_INVALID as the
 * export, with `entries` 8-byte aligned. Memory: the export's blocks, in host mode 40 bytes per kept entry. */
typedef struct svo_voxel_entry_dst {
    svo_voxel_segment *segments;    /* HOST memory always, >= n entries                                     */
    svo_voxel_entry   *entries;     /* host or device (mem), 8-byte aligned; NULL: every point_capacity is 0 */
} svo_voxel_entry_dst;

int svo_submit_save_voxel_maps(svo_ctx *ctx, const int *seqs, int n, const svo_voxel_region *regions,
                               const svo_voxel_filter *filter, const svo_voxel_entry_dst *dst, int mem);
int svo_save_voxel_maps(svo_ctx *ctx, const int *seqs, int n, const svo_voxel_region *regions,
                        const svo_voxel_filter *filter, const svo_voxel_entry_dst *dst, int mem);   /* submit + wait */

/* svo_submit_load_voxel_maps offers spans[i] (entries, n and voxel; `map` is not read) to the map of slot seqs[i]. The
 * entries lie in host or device memory (mem) and stay alive and unchanged until the wait; host entries are staged
 * through a block of the group. mode: SVO_VOXEL_LOAD_REPLACE clears the map first, counters to 0; SVO_VOXEL_LOAD_MERGE
 * does not. One merge launch per group. info[i] belongs to seqs[i], is host memory and is valid at svo_wait:
 *   SVO_VOXEL_LOADED       merged: the four counts of svo_voxel_merge_result; n_voxels: the map's entries afterwards,
 *                          from the header the job copies back, which is the new mirror
 *   SVO_VOXEL_LOAD_NO_MAP  the slot has no map (this comes first)
 *   SVO_VOXEL_LOAD_FULL    the load bound fails on the mirror (n_voxels taken as 0 for a replace): nothing changes, a
 *                          replace does not clear, the ctx does not fail; n_voxels: the mirror's
 * A fuse, prune or carve queued right behind a load is admitted on the loaded count. Rejected with SVO_ERR_INVALID
 * and nothing queued: a span svo_voxel_merge rejects, an unknown mode or mem, a NULL info, and a span whose voxel is
 * not bit for bit the edge of the slot's map as the ctx knows it then (maps change only through setters that wait
 * for the queues; a slot without a map is not checked). Memory, per group, made on first use: the fuse job's table
 * block (with 32 bytes more per slot) and in host mode 40 bytes per record of the job. */
enum { SVO_VOXEL_LOAD_REPLACE = 0, SVO_VOXEL_LOAD_MERGE = 1 };
enum { SVO_VOXEL_LOADED = 0, SVO_VOXEL_LOAD_NO_MAP = 1, SVO_VOXEL_LOAD_FULL = 2 };

typedef struct svo_voxel_load_info { /* 64 bytes, host, one per named slot */
    int32_t seq, run;               /* slot and ordinal of its run                                          */
    int32_t status;                 /* SVO_VOXEL_LOAD*                                                      */
    int32_t _pad;
    int64_t n_offered, n_merged, n_skipped, n_claimed;   /* as svo_voxel_merge_result; not loaded: 0        */
    int64_t n_voxels;               /* of the map after the job (NO_MAP: 0)                                 */
    int64_t _pad2;
} svo_voxel_load_info;

int svo_submit_load_voxel_maps(svo_ctx *ctx, const int *seqs, int n, const svo_voxel_entry_span *spans, int mode, int mem,
                               svo_voxel_load_info *info);
int svo_load_voxel_maps(svo_ctx *ctx, const int *seqs, int n, const svo_voxel_entry_span *spans, int mode, int mem,
                        svo_voxel_load_info *info);   /* submit + wait */

/* svo_ctx_resize_voxel_maps is a setter like svo_ctx_set_voxel_maps: it waits for the queues. Every named slot with a
 * map (seqs == NULL: every slot; slots without a map are skipped) gets a map of 1 << log2_capacity entries (10 .. 26)
 * with the same voxel and drop_flags that holds the old map's entries and counters (the rehash above); the old map
 * is released and svo_memory.device_bytes follows. Shrinking is allowed where it fits. If the entries of any named
 * slot do not fit the new capacity (the mirror's n_voxels > capacity' - capacity' / 4) the call is SVO_ERR_CAPACITY
 * before anything is allocated or changed. Then the new map of every slot that moves is allocated before any map is
 * moved: an allocation that fails gives the others back and leaves every map as it was too. Until the moves are done
 * the old and the new maps of the named slots exist side by side. */
int svo_ctx_resize_voxel_maps(svo_ctx *ctx, const int *seqs, int n, int log2_capacity);

/* ---- snapshots: the sequence state of a slot saved, loaded, moved between ctxs ------------
 * The reference has no checkpoint or resume (a StereoSlam lives and dies with its process). A snapshot is
 * everything the next frame of a slot depends on and everything its getters return, so that a sequence saved
 * after frame k and loaded into any slot of any compatible ctx (another process, GPU, group layout, solver mode,
 * input format, memory mode, template-ring size) gives from frame k+1 on exactly the frames of the uninterrupted
 * run. It has two parts:
 *
 * HOST PART (host memory always; little endian, every field 4-byte aligned, sections in this order, no gaps):
 *   header      struct svo_snapshot_info (160 bytes)
 *   pose filter the 12-state filter: statePre[12], statePost[12], then A, H, Q, R, errorCovPre, errorCovPost,
 *               gain, 144 floats each, row major (4128 bytes)
 *   frame       double time_stamp; float pose[6] (the filtered pose: svo_get_pose); svo_frame_stats: 616 bytes
 *   trajectory  n_trajectory x svo_pose
 *   keyframes   (n_keyframes - first_keyframe) x svo_snapshot_keyframe: the resident keyframes, oldest first
 *   directory   n_planes x svo_snapshot_plane: where every plane lies in the data part, in this order:
 *                 the current keypoint set: kps2d, kps3d, flags, keyframe_id, keypoint_index, outlier_count,
 *                   inlier_count, kf_inv_depth, kf_variance, score, level_type, color (12 planes of one row,
 *                   n_keypoints entries each); the colour generator's word (4 bytes); the keypoint count as the
 *                   device holds it (4 bytes)
 *                 per resident keyframe, retired ones included: the same 12 planes with the keyframe's n entries
 *                 per image set: left pyramid levels 0 .. pyramid_levels-1 (level l: (width >> l) x (height >> l)),
 *                   the right image, LK levels 1 .. lk_levels-1 (halved rounding up); rows = the image's,
 *                   row_bytes = its width
 *               Image set 0 is the current frame's; the others are those of the live keyframes in keyframe order,
 *               each stored once (a keyframe made on the current frame refers to set 0).
 * DATA PART (host or device memory: mem): the planes, rows dense (pitch = row_bytes), each at its directory
 *   offset (save puts them at multiples of 16; the bytes between planes are not written). No pointers anywhere.
 *
 * Not part of a snapshot: the slot's run ordinal and finished-run records, the counters of svo_totals: frames count where
 * they ran, the KLT template cache (a loaded slot's cache starts empty; results do not depend on it), the previous
 * frame's images (no later frame reads them), and every setting of the ctx. */
#define SVO_SNAPSHOT_MAGIC   0x534f5653u            /* "SVOS" */
#define SVO_SNAPSHOT_VERSION 1
#define SVO_SNAPSHOT_BYTE_ORDER 0x01020304u
enum { SVO_SNAPSHOT_COMPLETE = 0,
       SVO_SNAPSHOT_TOO_SMALL = 1 };  /* a capacity was too small when the save ran: only the header was written */

/* the header of a host part; also what svo_snapshot_info returns. (A struct tag only, no typedef: the function
 * of the same name.) */
struct svo_snapshot_info {
    uint32_t magic, version, byte_order;
    uint32_t status;                   /* SVO_SNAPSHOT_*                                                    */
    int64_t  host_bytes, data_bytes;   /* sizes of the two parts (TOO_SMALL: the sizes needed)              */
    svo_camera_settings cam;
    int32_t  width, height;
    int32_t  capacity;                 /* keypoints a slot can hold (svo_export_capacity)                   */
    int32_t  pyramid_levels, lk_levels;
    int32_t  frame_id;                 /* -1: the slot was empty (every count below is 0)                   */
    int32_t  n_keypoints;              /* of the current frame                                              */
    int32_t  n_trajectory;             /* frame_id + 1                                                      */
    int32_t  n_keyframes, keyframes_retired;   /* keyframes [0, retired) have given their images back        */
    int32_t  n_image_sets;
    int32_t  n_planes;                 /* 14 + 12 (n_keyframes - first_keyframe) + n_image_sets (pyramid_levels + lk_levels) */
    int32_t  first_keyframe;           /* keyframes below it were trimmed and are not in the snapshot: 0 <= first_keyframe
                                          <= keyframes_retired, n_keyframes - first_keyframe <= 4096 (0: untrimmed, the
                                          snapshot of earlier versions byte for byte)                        */
};
typedef struct svo_snapshot_keyframe {
    float   pose[6];
    int32_t n;                         /* its keypoints                                                     */
    int32_t image_set;                 /* which saved image set it uses; -1: retired                        */
} svo_snapshot_keyframe;
typedef struct svo_snapshot_plane {
    int64_t offset;                    /* in the data part                                                  */
    int32_t row_bytes, rows;           /* extent: rows x row_bytes bytes from there                         */
} svo_snapshot_plane;

/* the buffers of one snapshot. save: capacities in, written; load: the sizes of what is given, read. */
typedef struct svo_snapshot {
    void   *host;  int64_t host_capacity;     /* host part: host memory                                      */
    void   *data;  int64_t data_capacity;     /* data part: host (SVO_MEM_HOST) or device (SVO_MEM_DEVICE)   */
} svo_snapshot;

/* the sizes a save of the slot would need right now; a getter: waits for the queues */
int svo_snapshot_size(svo_ctx *ctx, int seq, int64_t *host_bytes, int64_t *data_bytes);
/* Save: snaps[i] receives slot seqs[i]. Queued like an export: it sees every frame set, restart and load submitted
 * before it and none submitted after; only the groups that own a named slot get work and no other group is
 * drained; the buffers stay valid until svo_wait, after which everything is delivered. The slot is not changed
 * (its deferred pose-filter update is flushed first, as the getters do). Level 0 and the right image are copied
 * even when they alias the caller's frames (SVO_MEM_DEVICE_BORROW, SBS_GRAY in place). An empty slot gives a valid
 * snapshot (frame_id -1). A capacity too small for the state when the save runs: only the header is written, with
 * the sizes needed and status SVO_SNAPSHOT_TOO_SMALL; nothing else is touched, the ctx does not fail and svo_wait
 * returns SVO_OK. Rejected with nothing queued (SVO_ERR_INVALID): an index out of range or named twice, a bad
 * mem, a null host part or host_capacity < sizeof(struct svo_snapshot_info), a null data part with
 * data_capacity > 0; a failed ctx, like svo_submit_images.
 * Host mode goes through one device staging block per group, made on first use and grown when outgrown
 * (svo_memory.device_bytes), and one copy per snapshot. A ctx that never saves or loads allocates nothing more
 * and adds no launch or copy to a step. */
int svo_submit_save(svo_ctx *ctx, const int *seqs, int n, svo_snapshot *snaps, int mem);
int svo_save_sequences(svo_ctx *ctx, const int *seqs, int n, svo_snapshot *snaps, int mem);   /* submit + wait */
/* Load: slot seqs[i] takes on snaps[i] (host_capacity / data_capacity: the bytes given). Queued like a save. The
 * slot first ends its current sequence exactly as svo_ctx_restart_sequences does (a finished-run record if it was
 * running), then takes the saved state into image sets and keyframe storage from the ctx's own free lists; the
 * images are the sets' own copies. Every getter then returns for the slot what it returned at the source when
 * the save ran; the slot keeps its own run ordinal. Loading an empty snapshot is a restart.
 * Compatibility: width, height and capacity must equal the ctx's, and the camera settings those of the target slot
 * (the header has the settings of the saved slot's rig; the target's: its rig as of this call, svo_ctx_assign_rigs
 * included) byte for byte; solver mode, input format, rectification maps, rig ids, memory mode, group count, slot
 * index, template-ring size and device are free; the resident keyframes (n_keyframes - first_keyframe) must fit the
 * ctx's keyframe table (svo_keyframe_range.table), else SVO_ERR_INVALID here, nothing queued or changed.
 * The host part is parsed and checked completely here, on the host, before anything is queued or changed: magic,
 * version, byte order, status, compatibility, every count against the capacity, every directory entry against
 * the extent its plane must have and the data part's size, the sizes against what was passed. A bad snapshot, an
 * index out of range or named twice, a bad mem: SVO_ERR_INVALID, nothing queued, every slot untouched, the ctx
 * usable. (The host part is copied at submit time: only the data part must stay valid until svo_wait.)
 * The DATA part is trusted as frames are: its bytes become keypoints and images unchecked. */
int svo_submit_load(svo_ctx *ctx, const int *seqs, int n, const svo_snapshot *snaps, int mem);
int svo_load_sequences(svo_ctx *ctx, const int *seqs, int n, const svo_snapshot *snaps, int mem);   /* submit + wait */
/* validates a host part (everything svo_submit_load checks but the compatibility with a ctx) and returns its
 * header; needs no GPU. A header-only part (SVO_SNAPSHOT_TOO_SMALL) of >= sizeof(struct svo_snapshot_info)
 * bytes is valid here (and rejected by a load). */
int svo_snapshot_info(const void *host_part, int64_t bytes, struct svo_snapshot_info *out);
/* stage entry of the copy kernel: n 2-D byte segments, device to device, in the tracker's launch (chunked when
 * the diagnostic SVO_SNAPSHOT_TABLE_TILES bounds the tile table). Of a segment exactly
 * [src + r * src_pitch, + row_bytes) is read for r in [0, rows) and the matching destination bytes are written;
 * rows or row_bytes of 0: nothing. Any addresses: 16 bytes per lane where source, destination and pitches allow,
 * dwords where 4-byte alignment allows, bytes otherwise. Negative sizes or pitches, a null pointer of a non-empty
 * segment, rows > 1 with dst_pitch < row_bytes: SVO_ERR_INVALID. Segments must not overlap each other's
 * destinations. */
typedef struct svo_copy_segment {
    const void *src;
    void       *dst;
    int64_t     row_bytes, rows;
    int64_t     src_pitch, dst_pitch;
} svo_copy_segment;
int svo_copy_segments(svo_handle *h, int n, const svo_copy_segment *segs);

/* per-frame diagnostics of the last svo_new_images call */
typedef struct svo_frame_stats {
    int32_t frame_id;
    int32_t is_keyframe;
    int32_t n_keypoints;
    int32_t n_keyframes;
    int32_t inside_count;
    int32_t overflow;
    float   pose_sia[6];
    float   pose_refined[6];
    float   sia_cost, reproj_cost;
    float   sia_ms;             /* device time of the sparse-alignment kernel (timing on) */
    float   stage_ms[8];        /* HIP-event times on the ctx stream (timing on): images+pyramids,
                                   compaction, sparse alignment, KLT, merge+reprojection GN,
                                   SSD disparity, filter update, keyframe phase + read-back */
    svo_gn_trace sia_trace[SVO_MAX_PYRAMID_LEVELS];
    svo_gn_trace reproj_trace;
} svo_frame_stats;
int svo_get_frame_stats(svo_ctx *ctx, int seq, svo_frame_stats *out);
/* counters accumulated over all sequences and all svo_new_images calls so far */
typedef struct svo_totals {
    int64_t frames;             /* sequence-frames processed                      */
    int64_t keyframes;          /* of which created a keyframe                    */
    int64_t keypoints;          /* sum of n_keypoints                             */
    int64_t gn_gradient_calls;  /* sum of get_gradient calls of the sparse alignment */
    int64_t gn_cost_calls;
    double  stage_ms[8];        /* sum of svo_frame_stats.stage_ms (timing on)    */
    double  wall_ms;            /* host wall time spent inside svo_new_images (max over groups) */
    int64_t launches;           /* frame sets processed, summed over groups: stage_ms / launches =
                                   mean duration of one stage launch                */
    int32_t n_groups;           /* independently driven sequence groups of the ctx */
    int32_t image_sets;         /* image sets (pyramids of one frame) allocated so far, summed over groups: bounded by
                                   the keyframes whose keypoints are still tracked (their images are released after that) */
} svo_totals;
int svo_get_totals(svo_ctx *ctx, svo_totals *out);
int svo_ctx_enable_timing(svo_ctx *ctx, int on);
int svo_ctx_set_fast_solver(svo_ctx *ctx, int on);  /* see svo_handle_set_fast_solver; default 0 */
int svo_ctx_set_exact_pinv(svo_ctx *ctx, int on);   /* older name: set_fast_solver(!on) */

/* The workgroup shapes the sparse alignment and the reprojection GN ran: one entry per distinct
 * (kernel, waves, mode, cap), with the number of group launches that used it, summed over the ctx's
 * groups since svo_ctx_create. Counted on the host where the shape is chosen. */
enum { SVO_KERNEL_SIA_GN = 0,       /* sia_gn_kernel<waves, mode>                                 */
       SVO_KERNEL_REPROJ_GN = 1 };  /* reproj_gn_kernel<waves> (mode 0)                           */
typedef struct svo_launch_shape {
    int32_t kernel;             /* SVO_KERNEL_*                                                   */
    int32_t waves;              /* wavefronts (64 lanes) per sequence                            */
    int32_t mode;               /* alignment: 0 records + image in LDS, 1 cost records in LDS,
                                   2 records and image taps from L2                               */
    int32_t cap;                /* keypoint slots per sequence                                    */
    int64_t launches;
} svo_launch_shape;
/* writes min(max, distinct shapes) entries (sorted by kernel, waves, mode, cap); *n = distinct shapes */
int svo_ctx_get_launch_shapes(svo_ctx *ctx, svo_launch_shape *out, int max, int *n);
/* the shapes a launch of `batch` sequences of at most n_bound keypoints would run, without a GPU:
 * out[0] the alignment (SVO_KERNEL_SIA_GN, workspaces of rec_cap keypoints, exact = reference-order
 * mode), out[1] the reprojection GN; launches = 1 if the keypoints fit the kernel, else 0 */
int svo_pick_launch_shapes(const svo_camera_settings *cam, int width, int height, int batch, int n_bound,
                           int rec_cap, int exact, svo_launch_shape out[2]);
/* the dynamic LDS (bytes per workgroup) the alignment kernel of that launch asks for (out[0] above) */
int svo_pick_sia_lds_bytes(const svo_camera_settings *cam, int width, int height, int batch, int n_bound,
                           int rec_cap, int exact, int64_t *lds_bytes);

/* ---- diagnostics (tests, not the tracking path) ----
 * n pseudo-inverses of 6x6 float systems H_dev[n][36] (row major, device) through the Jacobi SVD of
 * the Gauss-Newton solves: impl 0 = the sequential reference (one system per lane), 1 = the
 * lane-parallel solver of the kernels (one system per wavefront). out_dev[n][114] receives, per
 * system, Hinv[36], W[6], Vt[36] and U^T[36] (the scaled rows of At); sweeps_dev[n] the Jacobi
 * sweeps run (1..30). Both impls give the same bits. */
int svo_pinv6_check(svo_handle *h, const float *H_dev, int n, float *out_dev, int32_t *sweeps_dev, int impl);
/* Diagnostic: the exact Gauss-Newton solve delta = pinv(H) b of n systems (H_dev[n][36],
 * b_dev[n][6]), one wavefront each: impl 0 = the round-4 solve (wave-uniform finish, pseudo-inverse
 * and step), 1 = the lane-resident solve of the kernels. out_dev[n][120] receives Hinv[36], W[6],
 * Vt[36], U^T[36] and delta[6]; sweeps_dev[n] the Jacobi sweeps run. Both impls give the same bits. */
int svo_solve6_check(svo_handle *h, const float *H_dev, const float *b_dev, int n, float *out_dev,
                     int32_t *sweeps_dev, int impl);
/* Diagnostic: the alignment records (the per-level workspace svo_sparse_align's first kernel fills from the previous
 * frame: per patch pixel the reference half of the cost, the reference patch sum and the image gradient, per keypoint
 * sum g g^T) of `batch` sequences, computed by that kernel and by the one-lane-per-pixel kernel it replaced, on the
 * same inputs. kps2d / flags (NULL: none) hold the sequences `stride` entries apart, n_dev[batch] (device) the counts,
 * each 0..n_bound, n_bound <= stride; prev_pyr[batch][max_pyramid_levels] the level images (device; any base
 * alignment, stride >= width, at least 3 x 3; levels below min_pyramid_level_pose_estimation are not read). Each
 * kernel fills a workspace of its own, [batch][levels used][68][rec_cap] floats (rec_cap a multiple of 4, >= n_bound),
 * preset to ws_fill. *n_diff receives the number of 32-bit words in which the two differ, *first_diff the index of
 * the first (-1: none); rec_out (device, NULL: not wanted) the kernel's workspace, ref_out (likewise) the
 * replaced kernel's. */
int svo_sia_records_check(svo_handle *h, int batch, int stride, const int32_t *n_dev, int n_bound,
                          const svo_kp2d *kps2d, const uint32_t *flags, const svo_image *prev_pyr,
                          const svo_camera_settings *cam, int rec_cap, uint32_t ws_fill, float *rec_out,
                          float *ref_out, int64_t *n_diff, int64_t *first_diff);
/* Diagnostic: the reprojection refinement (svo_reproj_gn) of `batch` sequences in one launch, the way the
 * tracker launches it. Every keypoint array holds the sequences `stride` entries apart (sequence b starts at
 * b * stride); n_dev[batch] (device) the counts, each 0..n_bound, n_bound <= stride; pose_in / pose_out
 * [batch][6], cost [batch], trace [batch] (cost, trace, tracked + err may be NULL); zero_out [batch] or NULL:
 * every sequence's word is set to 0 (the tracker's inside counter). *waves and *cap receive the wavefronts
 * per sequence and the staged keypoint capacity that the launch chose for (batch, n_bound). Complete on return. */
int svo_reproj_gn_batch(svo_handle *h, int batch, int stride, const int32_t *n_dev, int n_bound, svo_kp2d *kps2d,
                        const svo_kp3d *kps3d, uint32_t *flags, const svo_camera_settings *cam,
                        const svo_kp2d *tracked, const float *err, const float *pose_in, float *pose_out,
                        float *cost, svo_gn_trace *trace, int32_t *zero_out, int *waves, int *cap);
/* Diagnostic: the sparse image alignment (svo_sparse_align) of `batch` sequences in one launch, the way the tracker
 * launches it. The keypoint arrays are laid out as above (n_dev[batch] device, each 0..n_bound, n_bound <= stride);
 * prev_pyr / cur_pyr: HOST arrays [batch][cam->max_pyramid_levels] of views onto device memory, every sequence its
 * own images, all of one width x height per level; pose_guess / pose_out [batch][6], cost [batch] or NULL, trace
 * [batch][SVO_MAX_PYRAMID_LEVELS] or NULL, dbg [batch][48] or NULL (H, b, step of the first get_gradient on
 * dbg_level). For the call every sequence gets record and per-keypoint workspaces of its own, and ws_fill is written
 * over all of them before the launch: what the kernel reads of a workspace slot that it did not write is this
 * pattern. *waves, *mode and *cap receive the shape the launch chose for (batch, n_bound). Complete on return. */
int svo_sparse_align_batch(svo_handle *h, int batch, int stride, const int32_t *n_dev, int n_bound,
                           const svo_kp2d *kps2d, const svo_kp3d *kps3d, const uint32_t *flags,
                           const svo_image *prev_pyr, const svo_image *cur_pyr, const svo_camera_settings *cam,
                           const float *pose_guess, int dbg_level, uint32_t ws_fill, float *pose_out, float *cost,
                           svo_gn_trace *trace, float *dbg, int *waves, int *mode, int *cap);
/* The same launch, and mats_out[batch] (device, 8-byte aligned) receives per sequence the block of rotation matrices
 * of its pose_out that the alignment kernel leaves for the tracker's KLT launch to project with. */
int svo_sparse_align_batch_mats(svo_handle *h, int batch, int stride, const int32_t *n_dev, int n_bound,
                                const svo_kp2d *kps2d, const svo_kp3d *kps3d, const uint32_t *flags,
                                const svo_image *prev_pyr, const svo_image *cur_pyr, const svo_camera_settings *cam,
                                const float *pose_guess, int dbg_level, uint32_t ws_fill, float *pose_out, float *cost,
                                svo_gn_trace *trace, float *dbg, int *waves, int *mode, int *cap, void *mats_out);
/* Host only: bytes of one such block and the offsets in it of Rd (double[9], cv::Rodrigues of the pose's rotation
 * vector r, row major), R (float[9], Rd rounded: PoseManager::get_rotation_matrix), Ri (float[9], cv::Rodrigues of -r
 * rounded: get_inv_rotation_matrix, src/lib/pose_manager.cpp:9-17) and t (float[3], the translation). Bytes outside
 * the four members are padding and hold nothing. Any output may be NULL. */
int svo_pose_mats_layout(int64_t *block_bytes, int64_t *rd_offset, int64_t *r_offset, int64_t *ri_offset,
                         int64_t *t_offset);
/* Diagnostic: the depth filter update (svo_depth_filter_update) of `batch` sequences in one launch, with explicit
 * references, laid out as above (kf_pose [batch * stride][6], frame_pose [batch][6]). do_flags: the counter
 * rules of StereoSlam::new_image (src/lib/stereo_slam.cpp:212-216) are applied to `flags`; do_reproject: kps2d
 * receives project_keypoints(frame_pose, kps3d) and inside_count[b] (or NULL; the caller zeroes it) is
 * increased by the keypoints of sequence b that KeyFrameManager::keyframe_needed counts in a width x height
 * image. Without a switch its outputs are not written. Complete on return. */
int svo_filter_update_batch(svo_handle *h, int batch, int stride, const int32_t *n_dev, int n_bound, svo_kp2d *kps2d,
                            svo_kp3d *kps3d, uint32_t *flags, const svo_camera_settings *cam,
                            const float *frame_pose, const float *disparity, const svo_kp3d *ref3d,
                            const svo_kp2d *ref2d, const float *kf_pose, int32_t *outlier_count,
                            int32_t *inlier_count, float *kf_inv_depth, float *kf_variance,
                            int do_outlier_check, int do_update, int do_flags, int do_reproject, int width,
                            int height, int32_t *inside_count);
/* Diagnostic: the KLT launch as the tracker makes it (svo_klt_track is the stage form: explicit start and reference
 * positions, no template cache). One launch of grid (n_bound, batch) over `batch` sequences; per sequence (HOST
 * array seqs[batch], every pointer in it device memory unless said otherwise):
 *   the start position of point i is project_keypoints(pose, kps3d[i]) with the sequence's own camera settings,
 *   computed in the kernel, from the rotation matrices of a one-thread launch (use_mats != 0) or from the pose alone;
 *   the reference position is kfs[kf_id[i]].kps2d[kp_index[i]] (kf_id NULL: keyframe 0 for every point);
 *   the template of (point, level) is read from / written to the keyframe's cache record (kp_index[i], level) when
 *   the keyframe has a cache (tmpl != NULL), the cache was made for this window (tmpl_win == win) and
 *   kp_index[i] < tmpl_cap; otherwise it is built and not kept.
 * The cache memory is the caller's: tmpl holds [tmpl_cap][SVO_LK_LEVELS] records laid out as svo_klt_cache_layout
 * says, tmpl_valid [tmpl_cap][SVO_LK_LEVELS] bytes (0: not stored yet; the kernel sets 1 when it stores a record).
 * tmpl_bytes / tmpl_valid_bytes are the sizes of the two blocks; the call is refused if a cache that the launch
 * would use is smaller than tmpl_cap records. The entry keeps nothing between calls.
 * Outputs per point: tracked, status, err (INFINITY where status is 0), proj_out (the projection), ref_out (the
 * gathered reference, or NULL). Entries [n, n_bound) of the outputs are not written. Before the launch the counts
 * (0 <= *n <= n_bound), kf_id (0 <= id < n_kfs) and kp_index (0 <= index < that keyframe's n_kps) are read back
 * and checked. win 3..35. Complete on return. */
typedef struct svo_klt_keyframe {
    svo_image lk[SVO_LK_LEVELS];    /* the keyframe's LK pyramid, views onto device memory                     */
    int32_t n_lk;                   /* 1..SVO_LK_LEVELS                                                          */
    int32_t n_kps;                  /* entries of kps2d                                                          */
    const svo_kp2d *kps2d;
    void *tmpl;                     /* or NULL: no cache                                                         */
    uint8_t *tmpl_valid;            /* or NULL with tmpl NULL                                                    */
    int64_t tmpl_bytes, tmpl_valid_bytes;
    int32_t tmpl_cap, tmpl_win;
} svo_klt_keyframe;
typedef struct svo_klt_sequence {
    const svo_klt_keyframe *kfs;    /* HOST array                                                                */
    int32_t n_kfs;                  /* 1..8                                                                      */
    int32_t n_cur;                  /* 1..SVO_LK_LEVELS                                                          */
    svo_image cur[SVO_LK_LEVELS];   /* the current frame's LK pyramid                                            */
    const int32_t *n;               /* [1] the number of points                                                  */
    const int32_t *kf_id;           /* [n] or NULL                                                               */
    const int32_t *kp_index;        /* [n]                                                                       */
    const svo_kp3d *kps3d;          /* [n]                                                                       */
    const float *pose;              /* [6]                                                                       */
    svo_camera_settings cam;
    svo_kp2d *tracked;              /* [n_bound] outputs ...                                                     */
    uint8_t *status;
    float *err;
    svo_kp2d *proj_out;
    svo_kp2d *ref_out;              /* ... or NULL                                                               */
} svo_klt_sequence;
int svo_klt_track_batch(svo_handle *h, int batch, const svo_klt_sequence *seqs, int n_bound, int win, int use_mats);
/* Host only: the layout of a keyframe's KLT template cache for window `win` (3..35). A cache of tmpl_cap keypoints
 * is tmpl_cap * *levels records of *record_bytes each, record (k, level) at ((k * *levels) + level) * *record_bytes,
 * and tmpl_cap * *levels flag bytes in the same order. A record is the template proper (one wavefront's 64 lanes x
 * 16 bytes per load, lane-major) and, at *header_offset, a header of *header_bytes: int32 state (0 reference window
 * outside the image, 1 flat, 2 trackable; only a trackable record's body is written), float A11, A12, A22,
 * double cI1, cI2. */
int svo_klt_cache_layout(int win, int64_t *record_bytes, int64_t *header_offset, int64_t *header_bytes, int *levels);

/* Diagnostics: the four bookkeeping launches of the keyframe path as the tracker makes them, on caller-made arrays.
 * Each entry takes a HOST array seqs[batch] (1 <= batch <= 4096) whose pointers are device memory, fills one
 * argument block per sequence the way the tracker's step fills it, launches once through the tracker's launcher,
 * and is complete on return; it keeps nothing between calls. The counts and indices a kernel would index with are
 * read back and checked before the launch (a diagnostic may wait).
 *
 * A keypoint set as the tracker holds it: twelve planes and a count, all device memory. */
typedef struct svo_kps_planes {
    svo_kp2d *kps2d;
    svo_kp3d *kps3d;
    uint32_t *flags;                /* SVO_IGNORE_* bits                                                         */
    int32_t  *kf_id, *kp_index, *outlier_count, *inlier_count;
    float    *kf_inv_depth, *kf_variance, *score;
    int32_t  *level_type;           /* level | type << 8                                                         */
    uint32_t *color;                /* r | g << 8 | b << 16                                                      */
    int32_t  *n;                    /* [1]                                                                       */
} svo_kps_planes;
/* Host only: the workgroup sizes the compaction launch of sets of `cap` keypoints and the select + merge launch of
 * `max_cells` candidates run with, and the bytes of "stored" flags a ctx gives a keyframe's template cache of
 * tmpl_cap keypoints (any of the outputs may be NULL). */
int svo_keyframe_launch_info(int cap, int max_cells, int tmpl_cap, int *compact_threads, int *merge_threads,
                             int64_t *tmpl_valid_bytes);
/* compact_kernel: src -> dst, order preserving, all twelve planes; *dst.n = the number kept.
 *   mode 0  remove_outliers (src/lib/stereo_slam.cpp:43-56): SVO_IGNORE_COMPLETELY goes
 *   mode 1  find_bad_keypoints (src/lib/depth_calculator.cpp:67-86) in a width x height image
 *   start   1: a sequence starts: nothing is copied, *dst.n = *src.n = 0 whatever *src.n held
 *   zero, zero_res: (or NULL) zero_count / zero_res_count words set to 0
 *   min_kf  (or NULL; mode 0 only, the entry refuses it with mode 1) [3]: the smallest kf_id among the keypoints kept
 *           (INT_MAX: none), then a 64-bit mask, low word first: bit j = a kept keypoint has kf_id min + j
 *   enable  (or NULL) [1]: 0 = the sequence's workgroup does nothing at all
 * Every plane holds `cap` entries; *src.n must be 0..cap unless start is set. *threads (or NULL) receives the
 * workgroup size launch_compact chose for cap. */
typedef struct svo_compact_sequence {
    svo_kps_planes src, dst;
    int32_t mode, width, height, start;
    const int32_t *enable;
    int32_t *zero, *zero_res, *min_kf;
    int32_t zero_count, zero_res_count;
} svo_compact_sequence;
int svo_compact_batch(svo_handle *h, int batch, const svo_compact_sequence *seqs, int cap, int *threads);
/* kf_select_merge_kernel: select_best_keypoints (src/lib/depth_calculator.cpp:37-65) over det[n_levels][max_cells]
 * with counts n_det[n_levels], then merge_keypoints (:88-130, grid arguments swapped as :179-180 does) into kps:
 * kps2d, score and level_type of the appended entries are written, *kps.n grows, clamped at cap with *overflow = 1
 * (it is not written otherwise); *old_count = the count before. sel, sel_level, sel_cell [max_cells] and occupied
 * [occupied_count >= the merge grid's cells] are workspaces. Checked: 0 <= n_det[i] <= max_cells, 0 <= *kps.n <= cap.
 * *threads: the workgroup size launch_select_merge chose for max_cells. */
typedef struct svo_merge_sequence {
    svo_camera_settings cam;
    int32_t width, height;
    const svo_det_cell *det;
    const int32_t *n_det;
    svo_kps_planes kps;
    svo_det_cell *sel;
    int32_t *sel_level, *sel_cell, *occupied;
    int32_t *old_count, *overflow;
    const int32_t *enable;
    int32_t occupied_count, pad_;
} svo_merge_sequence;
int svo_keyframe_merge_batch(svo_handle *h, int batch, const svo_merge_sequence *seqs, int n_levels, int max_cells,
                             int cap, int *threads);
/* kf_init_kernel: the depth and filter initialisation of keypoints [*old_count, *kps.n) (src/lib/depth_calculator.cpp:
 * 241-289, colours from the sequence's LCG state *color_lcg), the copy of the whole set and the pose into the new
 * keyframe's record (src/lib/keyframe_manager.cpp:15-32), and the ignore_temporary rules of src/lib/stereo_slam.cpp:
 * 157-159 and :237-245. kfs: the keyframe table, (kf_mask + 1) records of svo_keyframe_record_layout bytes, a ring:
 * record new_kf_id & kf_mask is written (planes = `record`, whose n is not used; tmpl, tmpl_valid, tmpl_cap,
 * tmpl_win; n and pose), record evict_id & kf_mask (evict_id >= 0) loses its tmpl pointer. tmpl_valid_bytes (a
 * multiple of 4) bytes at tmpl_valid are cleared. first_frame: zero pose (frame_pose is not read), LCG reseeded, no
 * keypoint stays temporary. *n_out = *kps.n. The planes of kps and record hold `cap` entries. Checked:
 * 0 <= *old_count <= *kps.n <= cap. */
typedef struct svo_kf_init_sequence {
    svo_camera_settings cam;
    int32_t first_frame, new_kf_id, kf_mask, evict_id;
    svo_kps_planes kps, record;
    const int32_t *old_count;
    const float *disparity, *frame_pose;
    void *kfs;
    int64_t kfs_bytes;
    uint32_t *color_lcg;
    int32_t *n_out;
    const int32_t *enable;
    void *tmpl;
    uint8_t *tmpl_valid;
    int32_t tmpl_valid_bytes, tmpl_cap, tmpl_win, pad_;
} svo_kf_init_sequence;
int svo_keyframe_init_batch(svo_handle *h, int batch, const svo_kf_init_sequence *seqs, int cap);
/* Host only: bytes of a keyframe table record and the offsets in it of its count (int32), pose (float[6]), template
 * cache pointer, "stored" flags pointer, tmpl_cap and tmpl_win (int32), and of the twelve plane pointers in the order
 * of the planes structure above. Any output may be NULL. */
int svo_keyframe_record_layout(int64_t *record_bytes, int64_t *n_offset, int64_t *pose_offset, int64_t *tmpl_offset,
                               int64_t *tmpl_valid_offset, int64_t *tmpl_cap_offset, int64_t *tmpl_win_offset,
                               int64_t plane_offsets[12]);
/* ssd_disparity_kernel as the tracker launches it: grid (n_bound, batch); sequence b handles keypoints
 * first + *first_ptr + 0 .. n_bound - 1 that lie below *n (first_ptr NULL: + 0); every other entry of disparity stays.
 * `win` and `search_y` choose the kernel shape (the tracker passes its settings); a sequence's own win, search_x
 * and search_y must not exceed win, 64 and search_y. kps2d and disparity hold `cap` entries. Checked: 0 <= *n <= cap,
 * and first, *first_ptr and n_bound each within 0..2^29 (their sum stays an int). *max_win: the largest window of the kernel shape launch_ssd chose (31 or 35). */
typedef struct svo_ssd_sequence {
    svo_image left, right;
    const int32_t *n;
    const svo_kp2d *kps2d;
    float *disparity;
    int32_t win, search_x, search_y, clamp_half;
    int32_t first, cap;
    const int32_t *first_ptr;
    const int32_t *enable;
} svo_ssd_sequence;
int svo_ssd_disparity_batch(svo_handle *h, int batch, const svo_ssd_sequence *seqs, int n_bound, int win, int search_y,
                            int *max_win);
/* Diagnostic: ssd_disparity_kernel (one wavefront per keypoint) against the four-wave kernel it replaced, which the
 * library keeps for this entry only. Both run on the same batch in svo_ssd_disparity_batch's launch form, with the
 * same checks; neither writes the sequences' own disparity arrays (which may be NULL). Each kernel writes into
 * [batch][stride] floats of its own, every word set to `fill` first, sequence b's entry i at b * stride + i
 * (stride >= every cap): an entry only one kernel writes differs, an entry neither wrote holds `fill`. *n_diff: the
 * number of 32-bit words that differ, *first_diff the index of the first (-1: none). disp_out / ref_out: NULL, or
 * device memory of batch * stride floats that receives the kernel's / the reference kernel's array. Complete on
 * return. */
int svo_ssd_disparity_check(svo_handle *h, int batch, const svo_ssd_sequence *seqs, int n_bound, int win, int search_y,
                            int stride, uint32_t fill, float *disp_out, float *ref_out, int64_t *n_diff,
                            int64_t *first_diff);

/* Diagnostic: the depth filter update as the tracker launches it for a tracked frame (svo_filter_update_batch is the
 * stage form: explicit references, nothing written outside the frame's arrays). Keypoint i of sequence b comes from
 * keyframe record kf_id[i] & kf_mask of the sequence's table (kf_mask = table - 1, table a power of two: a ring over
 * the ids, the tracker's form; kf_mask = -1: record kf_id[i] as it is), point kp_index[i] of it. The kernel
 *   gathers that record's pose, kps3d (the reference of DepthFilter::outlier_check) and kps2d (of update_kps3d),
 *   runs outlier_check and update_kps3d (src/lib/depth_filter.cpp:40-50) on the frame's own arrays, and
 *   with do_flags writes back into the keyframe as the loop of StereoSlam::new_image does
 *   (src/lib/stereo_slam.cpp:196-229): kps3d, outlier_count, inlier_count, and the flags merged: the keyframe keeps its
 *   own SVO_IGNORE_DURING_REFINEMENT bit and takes SVO_IGNORE_TEMPORARY and SVO_IGNORE_COMPLETELY from the frame;
 *   with do_reproject kps2d receives the projection and *inside_count (or NULL) is INCREASED by the keypoints that
 *   KeyFrameManager::keyframe_needed counts in a width x height image (src/lib/keyframe_manager.cpp:55-64).
 * Per sequence (HOST array seqs[batch]; every pointer device memory unless said otherwise): kps, the frame's set
 * (score, level_type and color are not used and may be NULL; the arrays hold at least *kps.n entries); kfs, a HOST
 * array of `table` keyframes, each its pose and five arrays of n entries (n 0: a vacant record, the arrays may be
 * NULL); records, `table` records of svo_keyframe_record_layout bytes that the entry fills before the launch (pose,
 * n and the five array pointers; everything else 0). Before anything is written the counts (0 <= *kps.n <= n_bound),
 * kf_id (>= 0, its record < table) and kp_index (0 <= index < that keyframe's n) are read back and checked. The pairs
 * (record, kp_index) of a sequence must be distinct, as they are in the reference (not checked: two keypoints of one
 * pair would race for the keyframe's entry). One launch of grid (ceil(n_bound / 64), batch), filled by the filling of
 * the tracker's step. Complete on return. */
typedef struct svo_filter_keyframe {
    float pose[6];
    svo_kp2d *kps2d;
    svo_kp3d *kps3d;
    uint32_t *flags;
    int32_t *outlier_count, *inlier_count;
    int32_t n, pad_;
} svo_filter_keyframe;
typedef struct svo_filter_table_sequence {
    svo_camera_settings cam;
    svo_kps_planes kps;
    const float *frame_pose;        /* [6]                                                                        */
    const float *disparity;         /* [n] (NULL without do_outlier_check)                                        */
    const svo_filter_keyframe *kfs; /* HOST array [table]                                                         */
    void *records;
    int64_t records_bytes;
    int32_t table, kf_mask, width, height;
    int32_t *inside_count;          /* [1] or NULL                                                                */
} svo_filter_table_sequence;
int svo_filter_update_table_batch(svo_handle *h, int batch, const svo_filter_table_sequence *seqs, int n_bound,
                                  int do_outlier_check, int do_update, int do_flags, int do_reproject);

#ifdef __cplusplus
}
#endif
#endif
