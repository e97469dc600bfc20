// What the facade test programs share: the files of a sequence directory and the records they write.
//   <dir>/cam.bin      svo_camera_settings
//   <dir>/meta.bin     int32 n_frames, width, height, n_samples
//   <dir>/ts.bin       float32 time stamp per frame
//   <dir>/frames.bin   per frame its buffer(s), rows packed: two gray images (pair), one 2W x H gray image (sbs),
//                      one W x H x 3 image (econ), two W x H x 3 images (bgr)
//   <dir>/samples.bin  update_pose samples, 88 bytes each (struct Sample)
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../stereo-svo-slam_amd/hostcpp/stereo_slam.hpp"

namespace facade_io {

using namespace svo_amd;

struct Sample {                // 88 bytes, no padding
    int32_t after_frame;      // applied after this frame
    int32_t first;            // 1: measures the frame's pose; 0: the pose the previous sample returned (the app's loop)
    float speed[6], pose_var[6], speed_var[6];
    double dt;
};
static_assert(sizeof(Sample) == 88, "Sample is 88 bytes");

inline std::vector<uint8_t> read_file(const std::string& path, size_t bytes) {
    std::vector<uint8_t> v(bytes);
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f || (bytes && std::fread(v.data(), 1, bytes, f) != bytes)) { std::printf("cannot read %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
    return v;
}

struct Sequence {
    CameraSettings cam;
    int n_frames = 0, w = 0, h = 0;
    std::vector<float> ts;
    std::vector<Sample> samples;
    std::vector<uint8_t> frames;
};

// bytes_per_pixel: of all buffers of one frame together (pair and sbs 2, econ 3, bgr 6)
inline Sequence read_sequence(const std::string& dir, size_t bytes_per_pixel) {
    Sequence s;
    const auto cb = read_file(dir + "/cam.bin", sizeof(s.cam));
    std::memcpy(&s.cam, cb.data(), sizeof(s.cam));
    int32_t meta[4];
    const auto mb = read_file(dir + "/meta.bin", sizeof(meta));
    std::memcpy(meta, mb.data(), sizeof(meta));
    s.n_frames = meta[0]; s.w = meta[1]; s.h = meta[2];
    if (s.n_frames < 1 || s.n_frames > 1000 || s.w < 1 || s.h < 1 || s.w > 8192 || s.h > 8192 || meta[3] < 0 || meta[3] > 100000) {
        std::printf("bad meta.bin\n");
        std::exit(2);
    }
    const auto tb = read_file(dir + "/ts.bin", sizeof(float) * s.n_frames);
    s.ts.resize(s.n_frames);
    std::memcpy(s.ts.data(), tb.data(), tb.size());
    const auto sb = read_file(dir + "/samples.bin", sizeof(Sample) * meta[3]);
    s.samples.resize(meta[3]);
    if (meta[3]) std::memcpy(s.samples.data(), sb.data(), sb.size());
    s.frames = read_file(dir + "/frames.bin", (size_t)s.n_frames * s.w * s.h * bytes_per_pixel);
    return s;
}

// a packed image of row_bytes x rows copied into rows of `step` bytes; the padding holds 0xA5
inline std::vector<uint8_t> with_step(const uint8_t* src, int row_bytes, int rows, int step) {
    std::vector<uint8_t> v((size_t)step * rows, 0xA5);
    for (int y = 0; y < rows; y++) std::memcpy(v.data() + (size_t)y * step, src + (size_t)y * row_bytes, row_bytes);
    return v;
}

inline void put(FILE* f, const void* p, size_t bytes) {
    if (bytes && std::fwrite(p, 1, bytes, f) != bytes) { std::printf("write failed\n"); std::exit(2); }
}
inline void put_i32(FILE* f, int32_t v) { put(f, &v, 4); }

// int32 n, then kps2d [n], kps3d [n], info [n]
inline void put_keypoints(FILE* f, const KeyPoints& k) {
    const size_t n = k.kps2d.size();
    if (k.kps3d.size() != n || k.info.size() != n) { std::printf("keypoint arrays of unequal length\n"); std::exit(2); }
    put_i32(f, (int32_t)n);
    put(f, k.kps2d.data(), sizeof(KeyPoint2d) * n);
    put(f, k.kps3d.data(), sizeof(KeyPoint3d) * n);
    put(f, k.info.data(), sizeof(KeyPointInformation) * n);
}

// int32 id, float32 pose [6] (PoseManager::get_vector), keypoints
inline void put_keyframe(FILE* f, const KeyFrame& kf) {
    put_i32(f, (int32_t)kf.id);
    const Vec6f p = kf.pose.get_vector();
    put(f, p.data(), sizeof(float) * 6);
    put_keypoints(f, kf.kps);
}

}  // namespace facade_io
