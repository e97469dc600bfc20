// The host-only types of the C++ facade (hostcpp/stereo_slam_types.hpp) in a program of their own: no GPU and no
// library to link. tests/test_facade_cpu.py builds it twice (plain, and with the address and undefined-behaviour
// sanitizers) and compares what it writes with the oracle's Rodrigues and the statement of tests/facade_ref.py.
//   pose_manager_check poses <in> <out>   <in>: float32[6] poses (x y z rx ry rz), or "-" for stdin
//       -> <out>: per pose 33 float32 (get_rotation_matrix 9, get_inv_rotation_matrix 9, get_robot_angles 3,
//          get_translation 3, get_angles 3, get_vector 6) and the text of operator<< in 128 bytes, NUL padded
//   pose_manager_check types              KeyFrameManager ids and look-ups, flags_of / set_flags; prints "types ok"
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../../stereo-svo-slam_amd/hostcpp/stereo_slam_types.hpp"

using namespace svo_amd;

static int fails = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } \
    } while (0)

static int run_poses(const char* in_path, const char* out_path) {
    FILE* in = std::strcmp(in_path, "-") == 0 ? stdin : std::fopen(in_path, "rb");
    FILE* out = std::fopen(out_path, "wb");
    if (!in || !out) { std::printf("cannot open %s / %s\n", in_path, out_path); return 2; }
    float p[6];
    int count = 0;
    while (std::fread(p, sizeof(float), 6, in) == 6) {
        const Pose pose{p[0], p[1], p[2], p[3], p[4], p[5]};
        PoseManager pm;
        if (count % 2) pm.set_vector({p[0], p[1], p[2], p[3], p[4], p[5]});      // both setters, alternating
        else pm.set_pose(pose);
        std::vector<float> rec;
        const Matx33f r = pm.get_rotation_matrix(), ri = pm.get_inv_rotation_matrix();
        const Vec3f ra = pm.get_robot_angles(), t = pm.get_translation(), a = pm.get_angles();
        const Vec6f v = pm.get_vector();
        rec.insert(rec.end(), r.begin(), r.end());
        rec.insert(rec.end(), ri.begin(), ri.end());
        rec.insert(rec.end(), ra.begin(), ra.end());
        rec.insert(rec.end(), t.begin(), t.end());
        rec.insert(rec.end(), a.begin(), a.end());
        rec.insert(rec.end(), v.begin(), v.end());
        const Pose back = pm.get_pose();
        if (std::memcmp(&back, &pose, sizeof(Pose)) != 0) { std::printf("get_pose differs at pose %d\n", count); return 1; }
        std::ostringstream os;
        os << pm;
        char text[128] = {0};
        const std::string s = os.str();
        if (s.size() >= sizeof(text)) { std::printf("text too long at pose %d\n", count); return 1; }
        std::memcpy(text, s.data(), s.size());
        if (std::fwrite(rec.data(), sizeof(float), rec.size(), out) != rec.size() || std::fwrite(text, 1, sizeof(text), out) != sizeof(text)) return 2;
        count++;
    }
    if (in != stdin) std::fclose(in);
    std::fclose(out);
    std::printf("poses %d\n", count);
    return 0;
}

static int run_types() {
    // a default PoseManager is the identity
    PoseManager pm;
    const Matx33f eye = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    EXPECT(pm.get_rotation_matrix() == eye && pm.get_inv_rotation_matrix() == eye);
    EXPECT((pm.get_vector() == Vec6f{0, 0, 0, 0, 0, 0}));

    // KeyFrameManager: ids 0, 1, 2 ... whatever id the keyframe came with; nullptr at and beyond size()
    CameraSettings cam{};
    KeyFrameManager m(cam);
    EXPECT(m.get_keyframe(0) == nullptr);
    std::vector<KeyFrame> got;
    m.get_keyframes(got);
    EXPECT(got.empty());
    for (int k = 0; k < 5; k++) {
        KeyFrame kf;
        kf.id = 100 + k;
        kf.time_stamp = 0.5 * k;
        kf.kps.kps2d.assign(k + 1, KeyPoint2d{(float)k, (float)-k});
        kf.pose.set_pose(Pose{(float)k, 0, 0, 0, 0.1f * k, 0});
        KeyFrame* added = m.add_keyframe(kf);
        EXPECT(added != nullptr && added->id == (uint64_t)k);
        EXPECT(m.get_keyframe((uint32_t)k) != nullptr && m.get_keyframe((uint32_t)k)->id == (uint64_t)k);
        EXPECT(m.get_keyframe((uint32_t)k + 1) == nullptr);
    }
    for (uint32_t id = 0; id < 5; id++) {
        KeyFrame* kf = m.get_keyframe(id);
        EXPECT(kf && kf->id == id && kf->kps.kps2d.size() == id + 1 && kf->time_stamp == 0.5 * id && kf->pose.get_pose().x == (float)id);
    }
    EXPECT(m.get_keyframe(5) == nullptr && m.get_keyframe(6) == nullptr && m.get_keyframe(0xffffffffu) == nullptr);
    // get_keyframes copies: changing the copy leaves the manager's keyframes alone, and the other way round
    m.get_keyframes(got);
    EXPECT(got.size() == 5);
    for (size_t k = 0; k < got.size(); k++) EXPECT(got[k].id == k && got[k].kps.kps2d.size() == k + 1);
    got[2].kps.kps2d.clear();
    got[2].id = 77;
    EXPECT(m.get_keyframe(2)->id == 2 && m.get_keyframe(2)->kps.kps2d.size() == 3);
    m.get_keyframe(3)->kps.kps2d[0].x = 42.f;
    EXPECT(got[3].kps.kps2d[0].x == 3.f);
    std::vector<KeyFrame> again(9);
    m.get_keyframes(again);
    EXPECT(again.size() == 5 && again[2].id == 2 && again[3].kps.kps2d[0].x == 42.f);

    // flags_of / set_flags: all eight combinations, whatever the record held before
    const uint32_t bits[3] = {SVO_IGNORE_DURING_REFINEMENT, SVO_IGNORE_COMPLETELY, SVO_IGNORE_TEMPORARY};
    EXPECT((bits[0] | bits[1] | bits[2]) == 7u);
    for (uint32_t before = 0; before < 8; before++)
        for (uint32_t f = 0; f < 8; f++) {
            KeyPointInformation i{};
            i.keyframe_id = 3; i.keypoint_index = 9; i.inlier_count = 4;
            set_flags(i, before);
            set_flags(i, f);
            EXPECT(flags_of(i) == f);
            EXPECT((i.ignore_during_refinement != 0) == ((f & bits[0]) != 0));
            EXPECT((i.ignore_completely != 0) == ((f & bits[1]) != 0));
            EXPECT((i.ignore_temporary != 0) == ((f & bits[2]) != 0));
            EXPECT(i.keyframe_id == 3 && i.keypoint_index == 9 && i.inlier_count == 4);
        }
    KeyPointInformation one{};
    one.ignore_completely = true;
    EXPECT(flags_of(one) == SVO_IGNORE_COMPLETELY);
    if (fails) return 1;
    std::printf("types ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[1], "poses") == 0) return run_poses(argv[2], argv[3]);
    if (argc == 2 && std::strcmp(argv[1], "types") == 0) return run_types();
    std::printf("usage: pose_manager_check poses <in|-> <out> | types\n");
    return 2;
}
