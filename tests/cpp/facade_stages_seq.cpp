// The stage classes of the C++ facade (PoseEstimator, project_keypoints, PoseRefiner with OpticalFlow inside,
// DepthFilter) on a frame whose keypoints come from more than one keyframe. StereoSlam runs over frames 0 .. K-1 of a
// sequence directory (tests/cpp/facade_io.hpp, the pair layout); the keyframes it made go into a KeyFrameManager, each
// with the pyramids of the frame it was made on; then the four classes run on frame K as StereoSlam::new_image chains
// them. tests/test_facade_gpu.py makes the same steps through the ctypes binding and compares bit for bit.
//   facade_stages_seq <dir> <K> [fast]
//   -> <dir>/stages.bin: int32 keyframes, int32 [keyframes] the frame each one appeared on, int32 n, then float32:
//      pose 6 + cost (alignment), pose 6 + cost (refinement), projected [n][2], tracked and merged kps2d [n][2],
//      updated kps3d [n][3], [n][5] (flags, outlier_count, inlier_count, kf_inv_depth, kf_variance)
#include "facade_io.hpp"

#include "../../stereo-svo-slam_amd/hostcpp/depth_filter.hpp"
#include "../../stereo-svo-slam_amd/hostcpp/pose_estimator.hpp"
#include "../../stereo-svo-slam_amd/hostcpp/pose_refinement.hpp"

using namespace svo_amd;
using namespace facade_io;

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    const int K = std::atoi(argv[2]);
    const bool fast = argc > 3 && std::string(argv[3]) == "fast";
    try {
        const Sequence seq = read_sequence(dir, 2);
        if (K < 1 || K >= seq.n_frames) { std::printf("bad frame %d\n", K); return 2; }
        const int w = seq.w, hgt = seq.h, step = w + 13;
        const size_t plane = (size_t)w * hgt;
        std::vector<std::vector<uint8_t>> lefts, rights;          // frames 0 .. K in rows of `step` bytes
        for (int k = 0; k <= K; k++) {
            lefts.push_back(with_step(seq.frames.data() + 2 * plane * k, w, hgt, step));
            rights.push_back(with_step(seq.frames.data() + 2 * plane * k + plane, w, hgt, step));
        }
        auto left_of = [&](int k) { return Image8{lefts[k].data(), w, hgt, step}; };
        auto right_of = [&](int k) { return Image8{rights[k].data(), w, hgt, step}; };

        // frames 0 .. K-1 through the tracker; a keyframe belongs to the frame on which get_keyframes grew
        StereoSlam slam(seq.cam);
        std::vector<int32_t> made_on;
        std::vector<KeyFrame> keyframes;
        for (int k = 0; k < K; k++) {
            slam.new_image(left_of(k), right_of(k), seq.ts[k]);
            slam.get_keyframes(keyframes);
            if (keyframes.size() > made_on.size() + 1) { std::printf("two keyframes on frame %d\n", k); return 4; }
            if (keyframes.size() > made_on.size()) made_on.push_back(k);
        }
        Frame previous;
        if (!slam.get_frame(previous)) return 4;

        Handle h(0, 4096);
        if (fast) check(svo_handle_set_fast_solver(h.get(), 1));
        KeyFrameManager keyframe_manager(seq.cam);
        for (size_t i = 0; i < keyframes.size(); i++) {
            keyframes[i].stereo_image = make_stereo_image(h, left_of(made_on[i]), right_of(made_on[i]), seq.cam);
            const KeyFrame* added = keyframe_manager.add_keyframe(keyframes[i]);
            if (added->id != i || keyframes[i].id != i) { std::printf("keyframe ids out of order\n"); return 4; }
        }
        previous.stereo_image = make_stereo_image(h, left_of(K - 1), right_of(K - 1), seq.cam);

        Frame frame;
        frame.id = (uint64_t)K;
        frame.kps = previous.kps;
        frame.stereo_image = make_stereo_image(h, left_of(K), right_of(K), seq.cam);

        PoseManager estimated;
        PoseEstimator estimator(h, frame.stereo_image, previous.stereo_image, previous.kps, seq.cam);
        const float sia_cost = estimator.estimate_pose(previous.pose, estimated);
        frame.pose = estimated;
        project_keypoints(h, frame.pose, frame.kps.kps3d, seq.cam, frame.kps.kps2d);
        const std::vector<KeyPoint2d> projected = frame.kps.kps2d;

        PoseRefiner refiner(h, seq.cam);
        const float refine_cost = refiner.refine_pose(keyframe_manager, frame);

        DepthFilter filter(h, keyframe_manager, seq.cam);
        std::vector<KeyPoint3d> updated;
        filter.update_depth(frame, updated);

        const int n = (int)frame.kps.kps2d.size();
        FILE* f = std::fopen((dir + "/stages.bin").c_str(), "wb");
        if (!f) return 2;
        put_i32(f, (int32_t)made_on.size());
        put(f, made_on.data(), 4 * made_on.size());
        put_i32(f, n);
        const Vec6f ps = estimated.get_vector(), pr = frame.pose.get_vector();
        put(f, ps.data(), 24); put(f, &sia_cost, 4);
        put(f, pr.data(), 24); put(f, &refine_cost, 4);
        put(f, projected.data(), 8 * (size_t)n);
        put(f, frame.kps.kps2d.data(), 8 * (size_t)n);
        put(f, updated.data(), 12 * (size_t)n);
        for (int i = 0; i < n; i++) {
            const KeyPointInformation& k = frame.kps.info[i];
            const float rec[5] = {(float)flags_of(k), (float)k.outlier_count, (float)k.inlier_count, k.kf_inv_depth, k.kf_variance};
            put(f, rec, sizeof(rec));
        }
        if (std::fclose(f) != 0) return 2;
        std::printf("keyframes %d keypoints %d sia_cost %.3f refine_cost %.4f\n", (int)made_on.size(), n, sia_cost, refine_cost);
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 3;
    }
    return 0;
}
