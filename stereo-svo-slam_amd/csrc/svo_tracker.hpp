// svo_tracker.hpp — device-side data layout of one tracked sequence and the
// argument blocks of the bookkeeping / keyframe kernels (keyframe.hip).
#pragma once

#include <vector>

#include "../../include/svo_hip.h"
#include "svo_kernels.hpp"
#include "svo_scene_plan.hpp"

namespace svo {

// Struct-of-arrays keypoint set in HBM (KeyPoints, src/include/stereo_slam_types.hpp:106-110;
// KeyPointInformation :85-98 split by field so that every kernel streams only
// the arrays it touches).
struct KpsDev {
    svo_kp2d* kps2d;
    svo_kp3d* kps3d;
    uint32_t* flags;
    int* kf_id;
    int* kp_index;
    int* outl;
    int* inl;
    float* kfx;        // depth filter state 1/z
    float* kfP;        // depth filter variance
    float* score;
    int* level_type;   // level | type << 8
    uint32_t* color;
    int* n;
};

// The depth filter's argument block in its tracker form (filter_update_kernel with FilterArgs::kfs set): the frame's
// keypoint set, its refined pose and disparities, the sequence's keyframe table (a ring of kf_mask + 1 records over the
// ids; -1: indexed by id as it is) and its inside counter, all four stages on. One filling for the tracker's step
// (pack_tracking_args) and for the diagnostic entry svo_filter_update_table_batch. `fa` must be cleared.
inline void fill_filter_table_args(FilterArgs& fa, const svo_camera_settings& cam, const KpsDev& k, const float* frame_pose,
                                   const float* disparity, KfDev* kfs, int kf_mask, int width, int height,
                                   int* inside_count) {
    fa.cam = cam; fa.n_ptr = k.n; fa.frame_pose = frame_pose;
    fa.kps2d = k.kps2d; fa.kps3d = k.kps3d; fa.flags = k.flags;
    fa.outlier_count = k.outl; fa.inlier_count = k.inl; fa.kf_inv_depth = k.kfx;
    fa.kf_variance = k.kfP; fa.disparity = disparity;
    fa.kfs = kfs; fa.kf_mask = kf_mask; fa.kf_id = k.kf_id; fa.kp_index = k.kp_index;
    fa.do_outlier_check = 1; fa.do_update = 1; fa.do_flags = 1; fa.do_reproject = 1;
    fa.width = width; fa.height = height; fa.inside_count = inside_count;
}

struct CompactArgs {
    KpsDev src, dst;
    int mode;          // 0: remove_outliers, 1: find_bad_keypoints
    int width, height;
    const int* enable; // optional device predicate
    int* zero;         // optional: zero_count ints set to 0 (the detection counters of the keyframe that follows)
    int zero_count;
    int start;         // 1: the first frame of a sequence: both keypoint sets are empty whatever their counts say (src.n is cleared too)
    int* zero_res;     // optional: zero_res_count ints set to 0 (the result block of a sequence that starts)
    int zero_res_count;
    int* min_kf;       // optional: [3] smallest origin-keyframe id among the keypoints kept (INT_MAX: none kept), then a 64-bit
                       // mask (low word first): bit j set = some kept keypoint comes from keyframe min + j (younger ones: not reported)
};
void launch_compact(const CompactArgs* d_args, int batch, int cap, hipStream_t stream);
int compact_pick_threads(int cap);                 // the workgroup size of that launch

struct DetCell {
    float x, y, score;
    int type;
};

struct DetectArgs {
    ImgView level[SVO_MAX_PYRAMID_LEVELS];
    int n_levels;      // left.size()/2
    int grid_w, grid_h;
    DetCell* out;      // [n_levels][max_cells]
    int* n_out;        // [n_levels]
    int max_cells;
    const int* enable;
};
// grid_w x grid_h: the level-0 cell of the launch's sequences (chooses the kernel shape)
void launch_detect(const DetectArgs* d_args, int batch, int max_cells, int n_levels, int grid_w, int grid_h, hipStream_t stream);
// the kernel shape launch_detect runs for that cell: its largest cell and the corners (of a cell + 1 px) its LDS list holds
struct DetectShape { int cell_w, cell_h, list; };
DetectShape detect_pick_shape(int grid_w, int grid_h);

struct MergeArgs {
    svo_camera_settings cam;
    int width, height;
    const DetCell* det;
    const int* n_det;
    int n_levels, max_cells;
    KpsDev kps;
    int cap;
    DetCell* sel;      // [max_cells]
    int* sel_level;    // [max_cells]
    int* sel_cell;     // [max_cells]
    int* occupied;     // [merge cells]
    int* old_count;
    int* overflow;
    const int* enable;
};
void launch_select_merge(const MergeArgs* d_args, int batch, int max_cells, hipStream_t stream);
int select_merge_pick_threads(int max_cells);      // the workgroup size of that launch

constexpr uint32_t SVO_COLOR_LCG_SEED = 12345u;   // state of a sequence's colour generator before its first keypoint

struct KfInitArgs {
    svo_camera_settings cam;
    KpsDev kps;
    const int* old_count;
    const float* disparity;
    const float* frame_pose;
    int first_frame;   // 1: frame 0 of a sequence: zero pose, no temporary flags, colour LCG reseeded (SVO_COLOR_LCG_SEED)
    int new_kf_id;
    int kf_mask;       // the table is a ring: keyframe id in record id & kf_mask
    KfDev* kfs;
    uint32_t* color_lcg;
    int* n_out;
    const int* enable;
    // the record of the new keyframe (written to kfs[new_kf_id] by the kernel: no copy of its own per keyframe),
    // the "stored" flags of its template cache block (cleared here) and the keyframe that loses the block (-1: none, or no longer in the table)
    KfDev record;
    int tmpl_valid_bytes;
    int evict_id;
};
void launch_kf_init(const KfInitArgs* d_args, int batch, hipStream_t stream);
// bytes of "stored" flags of a template cache block of tmpl_cap keypoints (kf_init_kernel clears them as dwords)
inline size_t kf_tmpl_valid_bytes(int tmpl_cap) { return ((size_t)tmpl_cap * SVO_LK_LEVELS + 255) / 256 * 256; }

// ------------------------------------------------------------ bulk export (export.hip)
// One tile of a keypoint set on its way into the records of the C ABI: at most EXPORT_TILE keypoints, one
// workgroup. The source arrays point at the tile's first keypoint (kps2d / kps3d as dwords; the ten 4-byte planes
// in the order flags, outlier count, inlier count, keyframe id, keypoint index, 1/z, variance, score,
// level | type << 8, colour); `first` is the record of every output array that keypoint goes to.
constexpr int EXPORT_TILE = 256;
constexpr int EXPORT_PLANES = 10;
struct ExportTile {
    const uint32_t* kps2d;
    const uint32_t* kps3d;
    const uint32_t* plane[EXPORT_PLANES];
    int64_t first;
    int count, pad_;
};
// keypoints [start, start + count) of the set, to records first + start ... (count <= EXPORT_TILE)
ExportTile export_tile(const KpsDev& k, int start, int count, int64_t first);
// every output array: device memory or null (skipped); nothing is launched for no tiles or no arrays
void launch_export(const ExportTile* d_tiles, int n_tiles, svo_kp2d* kps2d, svo_kp3d* kps3d, svo_kp_info* info,
                   hipStream_t stream);

// ------------------------------------------------------------ map export (map.hip)
// One tile of a keyframe's keypoint set on its way into the compacted points of a region: at most MAP_TILE
// keypoints, one workgroup. The planes point at the tile's first keypoint (kps3d as dwords). The tiles of a call
// are numbered in the order they are added (index): those of a region are consecutive, those of a set too, and
// tile_counts[index] receives the tile's kept points. A set without keypoints still has one tile (count 0), so that
// every set's count is written.
constexpr int MAP_TILE = 256;
struct MapTile {
    const uint32_t* kps3d;
    const uint32_t* flags;
    const int* kf_id;
    const int* inl;
    const uint32_t* color;
    int64_t first;         // record of `points` the tile's region starts at
    int count;             // keypoints of the tile
    int own_id;            // id of the keyframe that holds the set
    int index;             // of the tile in the call
    int region_tile;       // index of the first tile of its region
    int set_tile;          // index of the first tile of its set
    int set;               // >= 0: the tile is the last of set `set` (set_counts[set] is written); -1: it is not
};
// appends the tiles of keypoints [0, n) of set `set` of a region whose first tile has index region_tile
void map_tiles(const KpsDev& k, int n, int own_id, int set, int64_t first, int region_tile, std::vector<MapTile>& out);
// A chunk of a call's tiles, in index order and after every earlier chunk on the same stream: the count launch
// writes tile_counts[index] of the chunk's tiles, the write launch sums the counts of a tile's region before it,
// writes the kept points (points: device, 16-byte aligned, or null: none) and set_counts (or null).
void launch_map(const MapTile* d_tiles, int n_tiles, const svo_map_filter& filter, svo_map_point* points,
                int* tile_counts, int* set_counts, hipStream_t stream);

// ------------------------------------------------------------ segment copies (snapshot.hip)
// One tile of a 2-D byte segment: `rows` rows of `row_bytes` bytes, one workgroup. rows * row_bytes is at most
// COPY_TILE_BYTES (a single row piece: row_bytes is).
constexpr int COPY_TILE_BYTES = 32768;
struct CopyTile {
    const uint8_t* src;
    uint8_t* dst;
    int64_t src_pitch, dst_pitch;
    int row_bytes, rows;
};
// the tiles of one segment, appended to `out` (none for rows or row_bytes of 0)
void cut_copy_tiles(const void* src, void* dst, int64_t row_bytes, int64_t rows, int64_t src_pitch, int64_t dst_pitch,
                    std::vector<CopyTile>& out);
void launch_copy_tiles(const CopyTile* d_tiles, int n_tiles, hipStream_t stream);

// ------------------------------------------------------------ views (view.hip)
// One tile of an output image: at most VIEW_TILE_W x VIEW_TILE_H pixels at (x0, y0) of a w x h image, one
// workgroup. src: the gray plane (any base, src_stride >= w); dst: the image, rows dense (w * bytes per pixel);
// the four keypoint planes of the set the markers come from (n = 0: none, the planes may be null).
constexpr int VIEW_TILE_W = 64, VIEW_TILE_H = 16;
struct ViewTile {
    const uint8_t* src;
    uint8_t* dst;
    const svo_kp2d* kps2d;
    const uint32_t* flags;
    const int* level_type;
    const uint32_t* color;
    int src_stride, w, h;
    int x0, y0;
    int n;
};
// what a launch draws, from a checked svo_view_style: bytes per pixel, and per marker size (0: size, 1:
// size_temporary) the half extents of a cross (s / 2) and of a square ((int)(s * 0.8) / 2)
struct ViewParams {
    int level, bpp, markers;
    uint32_t drop_flags;
    int half_cross[2], half_square[2];
};
// what a view job and the stage entry check of a style alike (levels: 0 .. max_levels - 1 of the left plane)
int view_check_style(const svo_view_style* style, int max_levels, const char* who);
ViewParams view_params(const svo_view_style& style);
// the tiles of one image, appended to `out` (kps null: no markers)
void view_tiles(const ImgView& src, uint8_t* dst, const KpsDev* kps, int n, std::vector<ViewTile>& out);
void launch_view(const ViewTile* d_tiles, int n_tiles, const ViewParams& p, hipStream_t stream);

// ------------------------------------------------------------ scene (scene.hip)
// One keyframe set of an image: the five planes the points come from (4-byte aligned), its keypoints and the id of
// the keyframe that holds it
struct SceneSet {
    const uint32_t* kps3d;
    const uint32_t* flags;
    const int* kf_id;
    const int* inl;
    const uint32_t* color;
    int n, own_id;
};
// One output image: w x h pixels at dst, rows dense, seen through cam; its sets and lines (device tables)
struct SceneImage {
    svo_scene_camera cam;
    uint8_t* dst;
    const SceneSet* sets;
    const svo_scene_line* lines;
    int n_sets, n_lines;
    int w, h;
};
// One tile of an image: at most SCENE_TILE_W x SCENE_TILE_H pixels at (x0, y0), one workgroup
constexpr int SCENE_TILE_W = 64, SCENE_TILE_H = 16;
struct SceneTile {
    int image, x0, y0, _pad;
};
// what a launch draws, from a checked svo_scene_style
struct SceneParams {
    int bpp, point_size;
    uint32_t background;
    svo_map_filter filter;
};
// what a scene job, svo_scene_size and the stage entry check alike
int scene_check_style(const svo_scene_style* style, const char* who);
int scene_check_camera(const svo_scene_camera* cam, const char* who, int i);
SceneParams scene_params(const svo_scene_style& style);
// pitch and image_bytes of a cols x rows image of a checked style
void scene_shape(const svo_scene_style& style, int cols, int rows, int64_t* pitch, int64_t* image_bytes);
SceneSet scene_set(const KpsDev& k, int n, int own_id);
// the tiles of image `image` (w x h), appended to `out`
void scene_tiles(int image, int w, int h, std::vector<SceneTile>& out);
// the 8 world lines of a frustum (svo_scene_frustum) as records of class cls and colour rgb, appended to `out`
void scene_frustum_lines(const float pose[6], const float dims[3], uint32_t cls_rgb, std::vector<svo_scene_line>& out);
void launch_scene(const SceneTile* d_tiles, int n_tiles, const SceneImage* d_images, const SceneParams& p, hipStream_t stream);
// Cloud points ("scene clouds"). One piece of a span of records: at most SCENE_SPLAT_PIECE of them, shown in `image`,
// one workgroup of the splat pass (svo_scene_plan.hpp cuts the spans)
constexpr int SCENE_SPLAT_PIECE = SCENE_PLAN_PIECE;
struct SceneSpan {
    const svo_map_point* points;
    int image, n;
};
// d_planes[image]: the image's key plane uint64[h][w], all ones before the splat pass; null: an image without cloud
// points (no piece may name it). The splat pass, then the tile kernel that starts from the planes.
void launch_scene_splat(const SceneSpan* d_spans, int n_spans, const SceneImage* d_images, unsigned long long* const* d_planes,
                        const SceneParams& p, int point_size, hipStream_t stream);
void launch_scene_clouds(const SceneTile* d_tiles, int n_tiles, const SceneImage* d_images, unsigned long long* const* d_planes,
                         const SceneParams& p, hipStream_t stream);

// ------------------------------------------------------------ ar (ar.hip)
// The screen record of one (image, triangle), written by the first launch and walked by the second: the snapped
// vertices (4 sub-pixel bits), the camera depth of each, the shaded colour r << 16 | g << 8 | b and the pixels whose
// centres can lie inside, clipped to the image (bx0 > bx1: dropped, or nothing to draw). Four 16-byte words.
struct ArRecord {
    int X0, Y0, X1, Y1;
    int X2, Y2; float z0, z1;
    float z2; uint32_t rgb; int _pad[2];
    int bx0, by0, bx1, by1;
};
// One output image: the background plane (any base, src_stride >= w), the w x h image at dst (rows dense), seen
// through cam; its draws (device table; everything they point to is device memory) and its n_records records, the
// triangles of draw 0 first
struct ArImage {
    svo_ar_camera cam;
    const uint8_t* src;
    uint8_t* dst;
    const svo_ar_draw* draws;
    ArRecord* records;
    int src_stride, w, h, n_records;
};
// One workgroup of the first launch: triangles [t0, t0 + AR_THREADS) of draw `draw` of image `image`, whose records
// start at rec0
constexpr int AR_THREADS = 256;
struct ArSetup {
    int image, draw, t0, rec0;
};
// One tile of an image: at most AR_TILE_W x AR_TILE_H pixels at (x0, y0), one workgroup of the second launch
constexpr int AR_TILE_W = 64, AR_TILE_H = 16;
struct ArTile {
    int image, x0, y0, _pad;
};
// what the launches draw, from a checked svo_ar_style
struct ArParams {
    int bpp;
    float light[3];
    float ambient, near;
};
// what an ar job, svo_ar_size and the stage entry check alike
int ar_check_style(const svo_ar_style* style, const char* who);
int ar_check_camera(const svo_ar_camera* cam, const char* who, int i);
// an occluder of the stage entries (svo_render_ar_occluded, svo_voxel_carve): records == NULL (nothing else is read but _reserved), or
// step 1 .. 16, cols and rows > 0 and 16-byte aligned records
int ar_check_occluder(const svo_ar_occluder* o, const char* who, int i);
ArParams ar_params(const svo_ar_style& style);
// pitch and image_bytes of a cols x rows image of a checked style
void ar_shape(const svo_ar_style& style, int cols, int rows, int64_t* pitch, int64_t* image_bytes);
// the work of image `image`: its tiles (w x h) and the first launch's items of its draws, appended; returns the
// image's records
int ar_work(int image, int w, int h, const svo_ar_draw* draws, int n_draws, std::vector<ArSetup>& setup, std::vector<ArTile>& tiles);
void launch_ar_setup(const ArSetup* d_setup, int n_setup, const ArImage* d_images, const ArParams& p, hipStream_t stream);
void launch_ar(const ArTile* d_tiles, int n_tiles, const ArImage* d_images, const ArParams& p, hipStream_t stream);
// ar occlusion (include/svo_hip.h, "ar occlusion"). The occluder of one image, beside its ArImage (same index): the
// organized lattice (null: the image has none; cols, rows > 0 and step 1 .. 16 otherwise) and the image's two
// counters {covered, hidden}, zero before the launch, which the tile kernel adds to. 32 bytes.
struct ArOccluder {
    const svo_map_point* records;
    unsigned long long* counts;
    int cols, rows, step, _pad;
};
// what the occluded launch reads of a checked svo_ar_occlusion
struct ArOcclusion {
    int hidden, alpha;
    float margin;
    uint32_t drop_flags;
};
// the scalar fields of an occlusion (on, hidden, alpha, margin, the reserved words)
int ar_check_occlusion(const svo_ar_occlusion* o, const char* who);
ArOcclusion ar_occlusion(const svo_ar_occlusion& o);
// launch_ar with occluders: d_occluders[image] belongs to d_images[image]
void launch_ar_occluded(const ArTile* d_tiles, int n_tiles, const ArImage* d_images, const ArOccluder* d_occluders, const ArParams& p,
                        const ArOcclusion& o, hipStream_t stream);

// ------------------------------------------------------------ dense disparity (dense.hip)
// One image pair of a launch: the two gray planes (any base, strides >= w; both w x h), the planes at out (cols x rows
// floats each, dense; 4-byte aligned) and the baseline of SVO_DENSE_DEPTH. One table entry per image: a workgroup
// takes its image from blockIdx.y and computes its tile from blockIdx.x.
struct DenseImage {
    const uint8_t* left;
    const uint8_t* right;
    float* out;
    int left_stride, right_stride, w, h;
    float baseline;
    int _pad;
};
// what a launch computes, from a checked svo_disparity_style whose win / search_x / search_y are resolved
struct DenseParams {
    int value, step, win, search_x, search_y, cost;
    int band;          // lattice rows of a workgroup at most (dense_plan; the values do not depend on it)
};
// what a disparity job, svo_disparity_size and the stage entry check alike; win / search_x / search_y of 0 are taken
// from cam (null: a 0 is rejected) before the limits are checked, into *out
int dense_check_style(const svo_disparity_style* style, const svo_camera_settings* cam, const char* who, DenseParams* out);
// cols, rows, planes and image_bytes of a w x h image pair (any out pointer may be null); lr = 1: with the lr plane
void dense_shape(const DenseParams& p, int w, int h, int* cols, int* rows, int* planes, int64_t* image_bytes, int lr = 0);
// the workgroups of one w x h image: every launch's grid.x is the largest of its images'
int dense_tiles(const DenseParams& p, int w, int h);
// the band of a launch that would have so many workgroups with the full band (call before dense_tiles)
void dense_plan(DenseParams& p, long long workgroups_at_full_band);
// n images (<= DENSE_MAX_IMAGES), grid (tiles, n)
constexpr size_t DENSE_MAX_IMAGES = 65535;
void launch_dense(const DenseImage* d_images, int n, int tiles, const DenseParams& p, hipStream_t stream);

// ------------------------------------------------------------ left-right cross-check (dense.hip's mirrored kernel, lr.hip)
// One image pair of a checked launch: the two gray planes as in DenseImage; out: the reverse plane, rows x w floats
// (the disparity of the search from right column xr back into the left image, at [iy][xr]; -1: invalid), written by
// the reverse launch and read by the check launch; value: cols x rows floats, the forward disparity before the check
// launch and the value plane after it; lr: the lr plane (cols x rows floats), or null; the baseline of SVO_DENSE_DEPTH.
struct LrImage {
    const uint8_t* left;
    const uint8_t* right;
    float* out;
    float* value;
    float* lr;
    int left_stride, right_stride, w, h;
    float baseline;
    int _pad;
};
// what a check launch computes: value SVO_DENSE_DEPTH converts the surviving disparities; max_lr_diff 0: report only
struct LrParams {
    int value, step;
    float max_lr_diff;
};
// a checked svo_stereo_check (null: off): on, and the tolerance. cloud: max_lr_diff 0 with lr = 1 is rejected
struct LrCheck {
    int on = 0;
    float max_lr_diff = 0.f;
};
int lr_check_parse(const svo_stereo_check* check, bool cloud, const char* who, LrCheck* out);
// the bytes of one image's reverse plane (a multiple of 256)
inline size_t lr_reverse_bytes(int w, int h, int step) { return ((size_t)(h / step) * (size_t)w * 4 + 255) / 256 * 256; }
// the reverse search of n images (<= DENSE_MAX_IMAGES): the grid of launch_dense over the same images and params
// (value and cost of p are not read: the plane holds disparities)
void launch_dense_reverse(const LrImage* d_images, int n, int tiles, const DenseParams& p, hipStream_t stream);
// the check of n images, grid (lr_tiles of the largest lattice, n)
constexpr int LR_TILE = 1024;
constexpr int lr_tiles(int64_t points) { return (int)((points + LR_TILE - 1) / LR_TILE); }
void launch_lr_check(const LrImage* d_images, int n, int tiles, const LrParams& p, hipStream_t stream);
// the lattice form (include/svo_hip.h, "sgm cross-check"): out is cols x rows floats, the disparity of the mirrored
// pair's lattice point at [iy][ixm], and the check gathers ixm = min((w - 1 - xr) / step, cols - 1); left and right
// are not read
void launch_lr_check_lattice(const LrImage* d_images, int n, int tiles, const LrParams& p, hipStream_t stream);

// ------------------------------------------------------------ semi-global aggregation (dense.hip's cost-volume kernel, sgm.hip)
// One image pair of a cost-volume launch: the two gray planes as in DenseImage; vol: uint16 [rows][cols][D] with
// D = search_x + 1 (j fastest, dense); count: uint16 [rows][cols]. Both 2-byte aligned.
struct CostImage {
    const uint8_t* left;
    const uint8_t* right;
    uint16_t* vol;
    uint16_t* count;
    int left_stride, right_stride, w, h;
};
// the cost volumes of n images (<= DENSE_MAX_IMAGES): launch_dense's grid over the same images and params (value and
// cost of p are not read), search_x <= 63
void launch_dense_cost_volume(const CostImage* d_images, int n, int tiles, const DenseParams& p, int cost_cap, hipStream_t stream);
// the same over the mirrored, swapped planes Lm[y][u] = R[y][w - 1 - u], Rm[y][u] = L[y][w - 1 - u] of every image:
// the volume and count plane of the mirrored pair's lattice, which is the lattice "dense" gives it
void launch_dense_cost_volume_mirrored(const CostImage* d_images, int n, int tiles, const DenseParams& p, int cost_cap, hipStream_t stream);
// One volume of an aggregation: vol and count as above (count null: every point has D candidates), sum: the block of
// S, uint16 [rows][cols][D], written by the first launch and read by the second; out: the value plane and, with cost,
// the cost plane behind it (cols x rows floats each); the baseline of SVO_DENSE_DEPTH.
struct SgmImage {
    const uint16_t* vol;
    const uint16_t* count;
    uint16_t* sum;
    float* out;
    int cols, rows, D;
    float baseline;
};
// a checked svo_sgm_params with the value and cost of the style. reverse_from > 0: the table entries from that index
// on are the reverse volumes of a checked job: they write their disparity alone whatever value and cost say
struct SgmParams {
    int p1, p2, cost_cap, subpixel, value, cost;
    int reverse_from;
};
int sgm_check_params(const svo_sgm_params* sgm, const char* who, SgmParams* out);
constexpr int SGM_MAX_D = 64;
// the bytes of one volume or one block of S (a multiple of 256), and of one count plane
inline size_t sgm_volume_bytes(int cols, int rows, int D) { return ((size_t)cols * (size_t)rows * (size_t)D * 2 + 255) / 256 * 256; }
inline size_t sgm_count_bytes(int cols, int rows) { return ((size_t)cols * (size_t)rows * 2 + 255) / 256 * 256; }
// the bytes of the reverse disparity plane of a checked SGM map, and what one image of an SGM map stages in all:
// sums, volume and count plane, and with a check those of the mirrored pair and its disparity plane
inline size_t sgm_reverse_bytes(int cols, int rows) { return ((size_t)cols * (size_t)rows * 4 + 255) / 256 * 256; }
inline size_t sgm_slot_bytes(int cols, int rows, int D, bool checked) {
    const size_t one = 2 * sgm_volume_bytes(cols, rows, D) + sgm_count_bytes(cols, rows);
    return checked ? 2 * one + sgm_reverse_bytes(cols, rows) : one;
}
// the four paths and the value rule of n volumes (<= DENSE_MAX_IMAGES): two launches, rows then columns, ordered by
// the stream; max_cols / max_rows: the largest lattice of the table
void launch_sgm(const SgmImage* d_images, int n, int max_cols, int max_rows, const SgmParams& p, hipStream_t stream);

// ------------------------------------------------------------ dense point clouds (cloud.hip)
// One image of a launch: the left plane (the gray of a record), the disparity and cost planes of a search over its
// lattice (cols x rows floats each, dense: dense_disparity_kernel's with cost), where its records start, its tile
// counts (one int per tile of CLOUD_TILE lattice points; written by the count launch, read by the write launch), its
// kept count (null: not reported), the rig, the pose and 48 bytes for the pose's matrices. One table entry per image: a workgroup takes its image
// from blockIdx.y and its tile from blockIdx.x.
constexpr int CLOUD_TILE = 256;
struct CloudImage {
    const uint8_t* left;
    const float* disp;
    const float* best;
    svo_map_point* points;
    int* tile_counts;
    int* n_points;
    int left_stride, w, h;
    float baseline, fx, fy, cx, cy;
    float pose[6];
    float* mats;       // 12 floats of the image's own: the pose's float rotation matrix and translation (the count launch writes them, the write launch reads them)
};
// what a launch computes, from a checked svo_cloud_style whose win is resolved
// (sgm_cost = 1: the planes are an SGM map's, whose cost is per pixel already: max_mean_cost drops best > max_mean_cost * 4.0f)
struct CloudParams {
    int step, win, frame, layout;
    float min_disparity, max_depth, max_mean_cost;
    int sgm_cost;
};
// what a cloud job, svo_cloud_size and the stage entry check alike (win / search_x / search_y as dense_check_style):
// the search of the job into *search (a disparity plane and a cost plane), the rest into *out
int cloud_check_style(const svo_cloud_style* style, const svo_camera_settings* cam, const char* who, DenseParams* search, CloudParams* out);
constexpr int cloud_tiles(int64_t points) { return (int)((points + CLOUD_TILE - 1) / CLOUD_TILE); }
// n images (<= DENSE_MAX_IMAGES), grid (tiles, n) twice: the count launch, then the write launch
void launch_cloud(const CloudImage* d_images, int n, int tiles, const CloudParams& p, hipStream_t stream);

// ------------------------------------------------------------ batched pose filter (pose_filter.hip)
// n_states filter states, one lane each, POSE_FILTER_LANES per workgroup. State b runs samples
// [first[b], first[b + 1]) (clamped to [0, n_samples)) in order; a state without samples is neither read nor written.
// All pointers: device memory. state_in: statePost[12] | errorCovPost[144] per state; state_out: statePre[12] |
// statePost[12] | errorCovPre[144] | errorCovPost[144] | gain[144] per state (after the state's last sample);
// start_pose: [n_states][6], what a chained first sample measures; filtered: [n_samples][6] or null.
constexpr int POSE_FILTER_LANES = 64;
constexpr int POSE_FILTER_IN_FLOATS = 12 + 144;
constexpr int POSE_FILTER_OUT_FLOATS = 2 * 12 + 3 * 144;
struct PoseFilterArgs {
    int n_states, n_samples;
    const float* state_in;
    const float* start_pose;
    const int* first;             // [n_states + 1]
    const svo_pose_sample* samples;
    float* state_out;
    float* filtered;
};
void launch_pose_filter(const PoseFilterArgs& a, hipStream_t stream);

// ------------------------------------------------------------ voxel maps (voxel.hip)
// A map in device memory, 16-byte aligned: the header (256 bytes), the key plane (uint64[capacity], ~0: empty) and
// one 32-byte accumulator record per entry (count, sx, sy, sz, sr, sg, sb, last). The sizes and the host arithmetic
// are svo_voxel_plan.hpp's.
struct VoxelHeader {              // the first 64 of the header's 256 bytes; the rest is 0
    uint32_t magic;
    int32_t log2_capacity;
    float voxel;
    uint32_t drop_flags;
    unsigned long long n_voxels, n_fused, n_outside, overflow;
    uint32_t _pad[4];
};
static_assert(sizeof(VoxelHeader) == 64, "one 64-byte block");
struct VoxelMapDev {              // a map of a launch
    uint8_t* base;
    float voxel;
    int32_t log2_capacity;
    uint32_t drop_flags;
    int32_t _pad;
};
struct VoxelSpanDev {             // n > 0 records for maps[map]; tile0: the workgroups of the spans before it
    const svo_map_point* points;
    int64_t n;
    int64_t tile0;
    int32_t map;
    uint32_t stamp;
};
struct VoxelFilterDev { uint32_t min_count, min_stamp; };   // min_count >= 1
// empty entries and a header with zero counters
void launch_voxel_clear(const VoxelMapDev& map, hipStream_t stream);
// headers[i] = the header block of maps[i] (one launch, so that the host reads them with one copy)
void launch_voxel_headers(const VoxelMapDev* d_maps, int n, VoxelHeader* d_headers, hipStream_t stream);
// n_spans >= 1 spans of `tiles` workgroups in all into the maps they name. lane_atomics: every lane adds its own
// record to the entry its key's leader found, instead of one summed add per distinct key of a wavefront (the same
// table content; a diagnostic that the bench tool times).
void launch_voxel_fuse(const VoxelSpanDev* d_spans, int n_spans, int64_t tiles, const VoxelMapDev* d_maps, bool lane_atomics,
                       hipStream_t stream);
// tile_offsets[t] = kept entries of the tiles before t, tile_offsets[tiles] = all kept entries (two launches)
void launch_voxel_count(const VoxelMapDev& map, VoxelFilterDev f, int32_t* tile_offsets, hipStream_t stream);
// the temporary storage of the sort of n pairs
int voxel_sort_temp_bytes(size_t n, size_t* bytes);
// after launch_voxel_count with the same filter: the (key, entry) pairs of the n kept entries, sorted by key, as
// records points[0, n). keys_* / index_*: n values each.
int launch_voxel_extract(const VoxelMapDev& map, VoxelFilterDev f, const int32_t* tile_offsets, size_t n, uint64_t* keys_in,
                         uint64_t* keys_out, uint32_t* index_in, uint32_t* index_out, void* sort_temp, size_t sort_temp_bytes,
                         svo_map_point* points, hipStream_t stream);
// The keep rule of a prune (include/svo_hip.h, "voxel prune"): min_count >= 1; c: the centre voxel's three key parts;
// radius < 0: no box.
struct VoxelKeepDev {
    uint32_t min_count, min_stamp;
    int32_t c[3];
    int32_t radius;
    static constexpr bool carves = false;
};
// The map rebuilt in place from its kept entries, with no host read-back: count and scan (tile_offsets as
// launch_voxel_count's), stage, clear, reinsert and the header's n_voxels, six launches ordered by the stream.
// n_bound: an upper bound of the kept count (the header's n_voxels as the host knows it); staging: the
// voxel_prune_plan block of n_bound entries. When nothing leaves, only tile_offsets is written.
void launch_voxel_prune(const VoxelMapDev& map, VoxelKeepDev keep, int32_t* tile_offsets, uint8_t* staging, uint64_t n_bound,
                        hipStream_t stream);
// The carve of a checked call (include/svo_hip.h, "voxel carve"): the camera, the image size as floats, the occluder
// lattice (records == nullptr: no evidence anywhere) and the guards. drop_flags holds SVO_CLOUD_DROPPED too.
struct VoxelCarveDev {
    float view[12];
    float fx, fy, cx, cy;
    float w, h;
    float margin, near;
    const svo_map_point* records;
    int32_t cols, rows, step;
    uint32_t drop_flags;
    uint32_t max_last;
    int32_t ring;
};
// The rule of a carving rebuild: an entry stays iff `keep` keeps it and `carve` does not carve it. ballots: one word
// per wavefront of the count pass (VOXEL_TILE / 64 per tile), read by the stage pass (nullptr: a diagnostic form without
// them, whose stage pass evaluates the rule again); counters: n_tested, n_carved.
struct VoxelCarveRule {
    VoxelKeepDev keep;
    VoxelCarveDev carve;
    unsigned long long* ballots;
    unsigned long long* counters;
    static constexpr bool carves = true;
};
// launch_voxel_prune under a VoxelCarveRule: the counters are zeroed on the stream first, then the same six launches.
VoxelCarveDev voxel_carve_dev(const svo_voxel_carve_rule& carve, const svo_ar_camera& camera, int width, int height, const svo_map_point* records,
                              int cols, int rows, int step);
void launch_voxel_carve(const VoxelMapDev& map, const VoxelCarveRule& rule, int32_t* tile_offsets, uint8_t* staging, uint64_t n_bound,
                        hipStream_t stream);
// ---- voxel entries (include/svo_hip.h, "voxel entries")
struct VoxelEntrySpanDev {        // n > 0 entry records for maps[map]; tile0: the workgroups of the spans before it
    const svo_voxel_entry* entries;
    int64_t n;
    int64_t tile0;
    int32_t map;
    int32_t _pad;
};
struct VoxelMergeCounts { unsigned long long n_offered, n_merged, n_skipped, n_claimed; };   // of one map: svo_voxel_merge_result
// launch_voxel_extract with the raw entries in place of the points: the same pairs and sort launches, then one
// 40-byte record per kept entry, entries[0, n)
int launch_voxel_pack(const VoxelMapDev& map, VoxelFilterDev f, const int32_t* tile_offsets, size_t n, uint64_t* keys_in,
                      uint64_t* keys_out, uint32_t* index_in, uint32_t* index_out, void* sort_temp, size_t sort_temp_bytes,
                      svo_voxel_entry* entries, hipStream_t stream);
// n_spans >= 1 spans of `tiles` workgroups in all merged into the maps they name; counts[map] += what the launch did
// (the caller zeroes them)
void launch_voxel_merge(const VoxelEntrySpanDev* d_spans, int n_spans, int64_t tiles, const VoxelMapDev* d_maps, VoxelMergeCounts* d_counts,
                        hipStream_t stream);
// dst (any bytes) becomes the cleared map of its params, receives every entry of src and then src's n_voxels and
// three cumulative counters: three launches ordered by the stream. dst shares no byte with src.
void launch_voxel_rehash(const VoxelMapDev& src, const VoxelMapDev& dst, hipStream_t stream);

}  // namespace svo
