// cloud.hip — the lattice points of a dense disparity search as coloured 3-D points: triangulated as the reference
// triangulates a new keypoint (DepthCalculator::calculate_depth, depth_calculator.cpp:241-256, through the functions
// kf_init_kernel uses: kp_triangulate / kp_to_world, svo_device.hpp), filtered, coloured from the left plane and
// written as 16-byte svo_map_point records, compacted or organized, many images in one launch. The picture is stated
// exactly in include/svo_hip.h ("clouds"). The search itself is dense_disparity_kernel (dense.hip), unchanged: it has
// written a disparity and a cost plane per image before these kernels run.
//
// An image's cols * rows lattice points, in row-major order, are cut into tiles of CLOUD_TILE = 256; a workgroup takes
// one tile (blockIdx.x) of one image (blockIdx.y), a lane one lattice point. Two launches, as map.hip's:
//
//  * cloud_count_kernel evaluates the predicate and writes the tile's kept count to the image's tile_counts[tile]: a
//    64-bit __ballot per wave, popcount, the four waves through LDS. Tile 0 of an image also writes the pose's float
//    rotation matrix and translation (pose_mats: double sine and cosine, once per image and not once per tile).
//  * cloud_write_kernel sums the image's tile_counts before its tile (a strided loop over the workgroup and a
//    reduction), evaluates the predicate again, ranks the kept lanes (mbcnt of the ballot inside a wave, the waves
//    through LDS) and writes each kept point with one 16-byte store at before + rank. In the organized layout every
//    lane stores at its lattice index and only the image's last tile sums the counts, for n_points.
//
// The offsets are sums of what an earlier launch wrote: no workgroup waits for another, nothing is atomic, and the
// order (tile order, lane order) and so every byte is the same for any launch geometry.
//
// Loads: lane i reads float i of the tile's stretch of the disparity and cost planes (coalesced dwords; the planes
// are 4-byte aligned) and the gray byte of its own pixel (a gather with the lattice step between lanes, inside one
// image row per lattice row). About 9 B in and up to 16 B out per lattice point in the write launch, 8 B in in the
// count launch; 16 and 32 bytes of LDS; the roof is HBM.
//
// Bounds: of an image, floats [0, cols * rows) of the two planes and pixels (x, y) with x < w, y < h are read
// (x = ix * step + step / 2 <= (cols - 1) * step + step / 2 < w); tile_counts [0, tiles) are written; records
// [0, kept) (compact, kept <= cols * rows) or [0, cols * rows) (organized) are written.
#include "svo_host.hpp"
#include "svo_tracker.hpp"

namespace svo {

constexpr int CLOUD_THREADS = 256;
constexpr int CLOUD_WAVES = CLOUD_THREADS / 64;
static_assert(CLOUD_TILE == CLOUD_THREADS, "one lane per lattice point of a tile");
static_assert(sizeof(svo_map_point) == 16 && sizeof(svo_cloud_style) == 48 && sizeof(svo_cloud_segment) == 64 && sizeof(svo_cloud_src) == 96 &&
              sizeof(CloudImage) == 112, "record sizes");

int cloud_check_style(const svo_cloud_style* s, const svo_camera_settings* cam, const char* who, DenseParams* search, CloudParams* out) {
    if (!s) return svo_set_error(SVO_ERR_INVALID, "%s: no style", who);
    const svo_disparity_style ds = {SVO_DENSE_DISPARITY, s->step, s->win, s->search_x, s->search_y, 1, {0, 0}};
    DenseParams dp;
    if (const int rc = dense_check_style(&ds, cam, who, &dp)) return rc;
    if (s->frame != SVO_CLOUD_WORLD && s->frame != SVO_CLOUD_CAMERA) return svo_set_error(SVO_ERR_INVALID, "%s: frame %d", who, s->frame);
    if (s->layout != SVO_CLOUD_COMPACT && s->layout != SVO_CLOUD_ORGANIZED) return svo_set_error(SVO_ERR_INVALID, "%s: layout %d", who, s->layout);
    for (const float v : {s->min_disparity, s->max_depth, s->max_mean_cost})
        if (!(v >= 0.f) || !(v <= FLT_MAX)) return svo_set_error(SVO_ERR_INVALID, "%s: a filter value is negative or not finite", who);
    if (s->_reserved[0] != 0 || s->_reserved[1] != 0 || s->_reserved[2] != 0) return svo_set_error(SVO_ERR_INVALID, "%s: a _reserved is not 0", who);
    if (search) *search = dp;
    if (out) *out = CloudParams{dp.step, dp.win, s->frame, s->layout, s->min_disparity, s->max_depth, s->max_mean_cost, 0};
    return SVO_OK;
}

// lattice point k of the image: is it kept? Its pixel, disparity and (of a valid point) camera frame point come back.
__device__ __forceinline__ bool cloud_keep(const CloudImage& im, const CloudParams& p, int cols, int total, int k, int& x, int& y,
                                           float loc[3]) {
    x = 0; y = 0; loc[0] = loc[1] = loc[2] = 0.f;
    if (k >= total) return false;
    const int iy = k / cols, ix = k - iy * cols;
    x = ix * p.step + p.step / 2;
    y = iy * p.step + p.step / 2;
    const float disp = G(im.disp)[k], best = G(im.best)[k];
    if (disp < 0.f) return false;                          // (-1: invalid; a valid disparity is >= 0.5)
    kp_triangulate((float)x, (float)y, disp, im.fx, im.fy, im.cx, im.cy, im.baseline, loc);
    bool keep = true;
    if (p.min_disparity != 0.f && disp < p.min_disparity) keep = false;
    if (p.max_depth != 0.f && loc[2] > p.max_depth) keep = false;
    if (p.max_mean_cost != 0.f && p.sgm_cost) {            // (an SGM map: best is the sum of four paths of a cost per pixel)
        if (best > p.max_mean_cost * 4.0f) keep = false;
    } else if (p.max_mean_cost != 0.f) {
        const int wb = p.win / 2, wa = (p.win + 1) / 2;
        const int tw = min(im.w - 1, x + wa) - max(0, x - wb), th = min(im.h, y + wa) - max(0, y - wb);
        if (best > p.max_mean_cost * (float)(tw * th)) keep = false;
    }
    return keep;
}

__global__ __launch_bounds__(CLOUD_THREADS) void cloud_count_kernel(const CloudImage* __restrict__ images, const CloudParams p) {
    __shared__ int wave_n[CLOUD_WAVES];
    const CloudImage im = G(images)[blockIdx.y];
    const int cols = im.w / p.step, total = cols * (im.h / p.step);
    const int tile = blockIdx.x;
    if (tile >= cloud_tiles(total)) return;                // (the grid is sized for the launch's largest image)
    if (tile == 0 && threadIdx.x == 0 && p.frame == SVO_CLOUD_WORLD) {
        PoseMats pm;
        pose_mats(im.pose, pm);
        for (int i = 0; i < 9; i++) G(im.mats)[i] = pm.R[i];
        for (int i = 0; i < 3; i++) G(im.mats)[9 + i] = pm.t[i];
    }
    int x, y;
    float loc[3];
    const bool keep = cloud_keep(im, p, cols, total, tile * CLOUD_TILE + (int)threadIdx.x, x, y, loc);
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < CLOUD_WAVES; w++) n += wave_n[w];
        G(im.tile_counts)[tile] = n;
    }
}

__global__ __launch_bounds__(CLOUD_THREADS) void cloud_write_kernel(const CloudImage* __restrict__ images, const CloudParams p) {
    __shared__ int wave_before[CLOUD_WAVES], wave_n[CLOUD_WAVES];
    const CloudImage im = G(images)[blockIdx.y];
    const int cols = im.w / p.step, total = cols * (im.h / p.step);
    const int tiles = cloud_tiles(total), tile = blockIdx.x;
    if (tile >= tiles) return;
    const int i = threadIdx.x, lane = i & 63, wave = i >> 6;
    const bool organized = p.layout == SVO_CLOUD_ORGANIZED;
    // kept points of the image's tiles before this one (organized: only the last tile needs them, for n_points)
    int before = 0;
    if (!organized || tile == tiles - 1) {
        for (int j = i; j < tile; j += CLOUD_THREADS) before += G(im.tile_counts)[j];
        for (int o = 32; o > 0; o >>= 1) before += __shfl_down(before, o);
    }
    const int k = tile * CLOUD_TILE + i;
    int x, y;
    float loc[3];
    const bool keep = cloud_keep(im, p, cols, total, k, x, y, loc);
    const unsigned long long m = __ballot(keep);
    const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) {
        wave_before[wave] = before;
        wave_n[wave] = __popcll(m);
    }
    __syncthreads();
    int at = 0, kept = 0;
    for (int w = 0; w < CLOUD_WAVES; w++) {
        at += wave_before[w];
        kept += wave_before[w] + wave_n[w];
        if (w < wave) at += wave_n[w];
    }
    if (k < total && (keep || organized)) {
        svo_kp3d q{loc[0], loc[1], loc[2]};
        if (keep && p.frame == SVO_CLOUD_WORLD) {
            PoseMats pm;
            for (int j = 0; j < 9; j++) pm.R[j] = G(im.mats)[j];
            for (int j = 0; j < 3; j++) pm.t[j] = G(im.mats)[9 + j];
            q = kp_to_world(pm, loc);
        }
        const uint32_t gray = G(im.left)[(int64_t)y * im.left_stride + x];
        uint4 r;
        r.x = keep ? __float_as_uint(q.x) : 0u;
        r.y = keep ? __float_as_uint(q.y) : 0u;
        r.z = keep ? __float_as_uint(q.z) : 0u;
        r.w = gray * 0x010101u | (keep ? 0u : (uint32_t)SVO_CLOUD_DROPPED << 24);
        ((SVO_GP(uint4))im.points)[organized ? (int64_t)k : (int64_t)(at + rank)] = r;
    }
    if (i == 0 && tile == tiles - 1 && im.n_points) *G(im.n_points) = kept;
}

void launch_cloud(const CloudImage* d_images, int n, int tiles, const CloudParams& p, hipStream_t stream) {
    if (n <= 0 || tiles <= 0) return;
    hipLaunchKernelGGL(cloud_count_kernel, dim3(tiles, n), dim3(CLOUD_THREADS), 0, stream, d_images, p);
    hipLaunchKernelGGL(cloud_write_kernel, dim3(tiles, n), dim3(CLOUD_THREADS), 0, stream, d_images, p);
}

}  // namespace svo
