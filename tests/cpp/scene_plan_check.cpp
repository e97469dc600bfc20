// scene_plan_check.cpp — csrc/svo_scene_plan.hpp without a GPU: the spans an entry point accepts, the pieces of a span
// (disjoint, in order, exactly [0, n), each read through a real array so that the sanitizers see an index past it),
// the key plane's bytes and the chunks of a job. Prints "scene plan ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../stereo-svo-slam_amd/csrc/svo_scene_plan.hpp"

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

using namespace svo;

namespace {

// the pieces of a span of n records touch every record once, in order
void check_pieces(int64_t n) {
    std::vector<unsigned char> seen((size_t)(n > 0 ? n : 0), 0);
    int64_t next = 0, pieces = 0;
    scene_each_piece(n, [&](int64_t first, int count) {
        CHECK(first == next && count >= 1 && count <= SCENE_PLAN_PIECE);
        CHECK(first + count == n || count == SCENE_PLAN_PIECE);          // only the last piece is short
        for (int k = 0; k < count; k++) seen[(size_t)(first + k)]++;
        next = first + count;
        pieces++;
    });
    CHECK(next == (n > 0 ? n : 0) && pieces == scene_span_pieces(n));
    for (unsigned char v : seen) CHECK(v == 1);
}

// the chunks of n slots cover every slot once, in order, none larger than `chunk`
void check_chunks(int n, size_t chunk) {
    std::vector<int> seen((size_t)n, 0);
    int next = 0;
    scene_each_chunk(n, chunk, [&](int first, int count) {
        CHECK(first == next && count >= 1 && (size_t)count <= chunk);
        CHECK(first + count == n || (size_t)count == chunk);
        for (int k = 0; k < count; k++) seen[(size_t)(first + k)]++;
        next = first + count;
    });
    CHECK(next == n);
    for (int v : seen) CHECK(v == 1);
}

}  // namespace

int main() {
    // spans: n >= 0; with records a non-null, 16-byte aligned address
    CHECK(scene_span_ok(0, 0) && scene_span_ok(8, 0) && scene_span_ok(4096, 1) && scene_span_ok(16, INT64_C(1) << 40));
    CHECK(!scene_span_ok(4096, -1) && !scene_span_ok(0, -1) && !scene_span_ok(0, 1) && !scene_span_ok(4104, 1) && !scene_span_ok(4097, 7));
    // pieces
    CHECK(scene_span_pieces(-5) == 0 && scene_span_pieces(0) == 0 && scene_span_pieces(1) == 1);
    CHECK(scene_span_pieces(SCENE_PLAN_PIECE) == 1 && scene_span_pieces(SCENE_PLAN_PIECE + 1) == 2);
    CHECK(scene_span_pieces((INT64_C(1) << 40) + 1) == (INT64_C(1) << 30) + 1);                   // (no 32-bit step inside)
    for (int64_t n : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)SCENE_PLAN_PIECE - 1,
                      (int64_t)SCENE_PLAN_PIECE, (int64_t)SCENE_PLAN_PIECE + 1, (int64_t)90240, (int64_t)752 * 480})
        check_pieces(n);
    // key planes
    CHECK(scene_key_bytes(1, 1) == 256 && scene_key_bytes(32, 1) == 256 && scene_key_bytes(33, 1) == 512);
    CHECK(scene_key_bytes(640, 480) == (size_t)640 * 480 * 8 && scene_key_bytes(4096, 4096) == (size_t)1 << 27);
    CHECK(scene_key_bytes(96, 40) == 30720 && scene_key_bytes(63, 15) % 256 == 0 && scene_key_bytes(63, 15) >= (size_t)63 * 15 * 8);
    // chunks: 256 MiB over the per-slot bytes, at least one slot, at most the named ones, lowered by the diagnostic
    const size_t MiB = (size_t)1 << 20;
    CHECK(scene_chunk_slots(MiB, 1000, 0) == 256 && scene_chunk_slots(MiB, 100, 0) == 100 && scene_chunk_slots(MiB, 0, 0) == 1);
    CHECK(scene_chunk_slots(300 * MiB, 7, 0) == 1 && scene_chunk_slots(0, 5, 0) == 5 && scene_chunk_slots(129 * MiB, 7, 0) == 1);
    CHECK(scene_chunk_slots(128 * MiB, 7, 0) == 2 && scene_chunk_slots(MiB, 1000, 3) == 3 && scene_chunk_slots(MiB, 2, 3) == 2);
    CHECK(scene_chunk_slots(MiB, 1000, -4) == 256 && scene_chunk_slots(MiB, 1000, 100000) == 256);
    for (int n : {0, 1, 2, 5, 7, 64})
        for (size_t chunk : {(size_t)1, (size_t)2, (size_t)3, (size_t)5, (size_t)64, (size_t)1000}) check_chunks(n, chunk);
    std::printf("scene plan ok\n");
    return 0;
}
