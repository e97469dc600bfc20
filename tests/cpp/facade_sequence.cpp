// Drives svo_amd::StereoSlam (hostcpp/stereo_slam.hpp) over a whole sequence, frame by frame, the way an integrator
// would, and writes everything it returns; tests/test_facade_gpu.py compares that with oracle_py.Slam.
//   facade_sequence <dir> <mode>          (the files of <dir>: tests/cpp/facade_io.hpp)
//   pair       Image8 left and right, step = cols + 13
//   sbs        set_input_format(SVO_INPUT_SBS_GRAY) before the first image, one buffer per frame
//   econ       SVO_INPUT_CH3_ECON through the Image8C3 overload
//   bgr        SVO_INPUT_BGR_PAIR through the two-image overload, step in bytes
//   fast       pair with set_fast_solver(true) before the first frame
//   fast_late  pair with set_fast_solver(true) after the third frame
// -> stdout: one line "null <call>: <exception text>" per call made before the first image, then "frames <n>"
// -> <dir>/out.bin:
//   int32 get_frame's return before the first image
//   per frame: int32 get_frame's return, int32 Frame::id, float64 time_stamp, float32 pose [6] (frame.pose.get_vector()),
//              keypoints (int32 n, kps2d, kps3d, info), int32 get_keyframes().size(), int32 m, float32 [m][6] update_pose returns
//   int32 count, then every keyframe of get_keyframes (int32 id, float32 pose [6], keypoints); get_keyframe's one;
//   int32 n, float32 [n][6] get_trajectory
#include <functional>

#include "facade_io.hpp"

using namespace svo_amd;
using namespace facade_io;

static void expect_throw(const char* name, const std::function<void()>& call) {
    try {
        call();
        std::printf("null %s: no exception\n", name);
    } catch (const std::runtime_error& e) {
        std::printf("null %s: %s\n", name, e.what());
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const std::string dir = argv[1], mode = argv[2];
    const bool pair = mode == "pair" || mode == "fast" || mode == "fast_late";
    if (!pair && mode != "sbs" && mode != "econ" && mode != "bgr") { std::printf("unknown mode %s\n", mode.c_str()); return 2; }
    try {
        const Sequence seq = read_sequence(dir, pair || mode == "sbs" ? 2 : (mode == "econ" ? 3 : 6));
        const int w = seq.w, h = seq.h;
        FILE* out = std::fopen((dir + "/out.bin").c_str(), "wb");
        if (!out) return 2;

        StereoSlam slam(seq.cam);
        Frame frame;
        put_i32(out, slam.get_frame(frame) ? 1 : 0);
        // no ctx yet: the C entries reject a NULL ctx (svo_ctx.hip, ctx_seq) and the facade passes that on
        const float zeros[6] = {0, 0, 0, 0, 0, 0};
        expect_throw("get_keyframe", [&] { KeyFrame kf; slam.get_keyframe(kf); });
        expect_throw("get_keyframes", [&] { std::vector<KeyFrame> kfs; slam.get_keyframes(kfs); });
        expect_throw("get_trajectory", [&] { std::vector<Pose> t; slam.get_trajectory(t); });
        expect_throw("update_pose", [&] { slam.update_pose(Pose{}, zeros, zeros, zeros, 0.01); });

        if (mode == "fast") slam.set_fast_solver(true);
        if (mode == "sbs") slam.set_input_format(SVO_INPUT_SBS_GRAY);
        if (mode == "econ") slam.set_input_format(SVO_INPUT_CH3_ECON);
        if (mode == "bgr") slam.set_input_format(SVO_INPUT_BGR_PAIR);

        const size_t plane = (size_t)w * h;
        for (int k = 0; k < seq.n_frames; k++) {
            if (mode == "fast_late" && k == 3) slam.set_fast_solver(true);
            if (pair) {
                const uint8_t* a = seq.frames.data() + 2 * plane * k;
                const auto l = with_step(a, w, h, w + 13), r = with_step(a + plane, w, h, w + 13);
                slam.new_image(Image8{l.data(), w, h, w + 13}, Image8{r.data(), w, h, w + 13}, seq.ts[k]);
            } else if (mode == "sbs") {
                const auto f = with_step(seq.frames.data() + 2 * plane * k, 2 * w, h, 2 * w + 13);
                slam.new_image(Image8{f.data(), 2 * w, h, 2 * w + 13}, 1, seq.ts[k]);
            } else if (mode == "econ") {
                const auto f = with_step(seq.frames.data() + 3 * plane * k, 3 * w, h, 3 * w + 13);
                slam.new_image(Image8C3{f.data(), w, h, 3 * w + 13}, seq.ts[k]);
            } else {
                const uint8_t* a = seq.frames.data() + 6 * plane * k;
                const auto l = with_step(a, 3 * w, h, 3 * w + 13), r = with_step(a + 3 * plane, 3 * w, h, 3 * w + 13);
                slam.new_image(Image8{l.data(), w, h, 3 * w + 13}, Image8{r.data(), w, h, 3 * w + 13}, seq.ts[k]);
            }
            const bool got = slam.get_frame(frame);
            put_i32(out, got ? 1 : 0);
            put_i32(out, (int32_t)frame.id);
            put(out, &frame.time_stamp, sizeof(double));
            const Vec6f pv = frame.pose.get_vector();
            put(out, pv.data(), sizeof(float) * 6);
            put_keypoints(out, frame.kps);
            std::vector<KeyFrame> kfs;
            slam.get_keyframes(kfs);
            put_i32(out, (int32_t)kfs.size());
            // the app's IMU loop: the first sample measures the frame's pose, the next ones what update_pose returned
            std::vector<Pose> returned;
            Pose prev = frame.pose.get_pose();
            for (const Sample& sm : seq.samples) {
                if (sm.after_frame != k) continue;
                prev = slam.update_pose(sm.first ? frame.pose.get_pose() : prev, sm.speed, sm.pose_var, sm.speed_var, sm.dt);
                returned.push_back(prev);
            }
            put_i32(out, (int32_t)returned.size());
            put(out, returned.data(), sizeof(Pose) * returned.size());
        }

        std::vector<KeyFrame> keyframes;
        slam.get_keyframes(keyframes);
        put_i32(out, (int32_t)keyframes.size());
        for (const KeyFrame& kf : keyframes) put_keyframe(out, kf);
        KeyFrame last;
        slam.get_keyframe(last);
        put_keyframe(out, last);
        std::vector<Pose> trajectory;
        slam.get_trajectory(trajectory);
        put_i32(out, (int32_t)trajectory.size());
        put(out, trajectory.data(), sizeof(Pose) * trajectory.size());
        if (std::fclose(out) != 0) return 2;
        std::printf("frames %d keyframes %d\n", seq.n_frames, (int)keyframes.size());
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 3;
    }
    return 0;
}
