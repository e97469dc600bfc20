// svo_ctx_snapshot.hip — the queued jobs of the ctx (svo_ctx_state.hpp) that change a slot's state from outside: save
// and load of snapshots with svo_snapshot_size, and the pose-filter updates.
#include "svo_ctx_state.hpp"

namespace {

// what svo_submit_save and svo_submit_load check alike, before anything is queued
int check_snapshot_call(svo_ctx* c, const char* name, const int* seqs, int n, const svo_snapshot* snaps, int mem) {
    if (!c || n < 0 || (n > 0 && (!seqs || !snaps)) || !mem_ok(mem))
        return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments (mem %d)", name, mem);
    return check_slots(c, name, NamedSlots{seqs, n});
}

}  // namespace

extern "C" int svo_submit_save(svo_ctx* c, const int* seqs, int n, svo_snapshot* snaps, int mem) {
    if (const int rc = check_snapshot_call(c, "svo_submit_save", seqs, n, snaps, mem)) return rc;
    for (int i = 0; i < n; i++)
        if (!snaps[i].host || snaps[i].host_capacity < (int64_t)sizeof(struct svo_snapshot_info) || snaps[i].data_capacity < 0 ||
            (!snaps[i].data && snaps[i].data_capacity > 0))
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_save: snapshot %d: the host part needs room for its header, the data part its memory", i);
    if (c->failed.load()) return reject_failed(c, "svo_submit_save");
    submit_shares<svo_ctx::Save>(c, NamedSlots{seqs, n}, [&](svo_ctx::Save& job, int i, int) { job.snaps.push_back(snaps[i]); return true; },
                                 [&](svo_ctx::Save& job) { job.mem = mem; });
    return SVO_OK;
}

extern "C" int svo_save_sequences(svo_ctx* c, const int* seqs, int n, svo_snapshot* snaps, int mem) {
    return then_wait(c, svo_submit_save(c, seqs, n, snaps, mem));
}

extern "C" int svo_submit_load(svo_ctx* c, const int* seqs, int n, const svo_snapshot* snaps, int mem) {
    if (const int rc = check_snapshot_call(c, "svo_submit_load", seqs, n, snaps, mem)) return rc;
    // every snapshot is parsed and checked before any group gets work
    std::vector<SnapshotLoad> loads((size_t)n);
    for (int i = 0; i < n; i++) {
        loads[i].seq = seqs[i];
        loads[i].data = snaps[i].data;
        if (const int rc = grp_check_snapshot(c->workers[0]->g.get(), &c->rigs[c->slot_rig[seqs[i]]].cam, &snaps[i], &loads[i].host))
            return rc;                           // (every group has the same size and capacity; the settings: the slot's rig's)
    }
    if (c->failed.load()) return reject_failed(c, "svo_submit_load");
    submit_shares<svo_ctx::Load>(c, NamedSlots{seqs, n}, [&](svo_ctx::Load& job, int i, int local) {
        loads[i].seq = local;
        job.loads.push_back(std::move(loads[i]));
        return true;
    }, [&](svo_ctx::Load& job) { job.mem = mem; });
    return SVO_OK;
}

extern "C" int svo_load_sequences(svo_ctx* c, const int* seqs, int n, const svo_snapshot* snaps, int mem) {
    return then_wait(c, svo_submit_load(c, seqs, n, snaps, mem));
}

extern "C" int svo_snapshot_size(svo_ctx* ctx, int seq, int64_t* host_bytes, int64_t* data_bytes) {
    svo_group* g; int s;
    if (const int rc = ctx_seq(ctx, seq, &g, &s)) return rc;
    return grp_snapshot_size(g, s, host_bytes, data_bytes);
}

extern "C" int svo_submit_pose_updates(svo_ctx* c, const int* seqs, const int* counts, int n, const svo_pose_sample* samples,
                                       float* filtered) {
    if (!c || !counts || !naming_ok(seqs, n)) return svo_set_error(SVO_ERR_INVALID, "svo_submit_pose_updates: bad arguments");
    const NamedSlots slots = ctx_slots(c, seqs, n);
    std::vector<int64_t> first((size_t)slots.n + 1, 0);     // sample offsets of the named slots
    const int rc = check_slots_and_items(c, "svo_submit_pose_updates", slots, [&](int i) {
        if (counts[i] < 0) return svo_set_error(SVO_ERR_INVALID, "svo_submit_pose_updates: sequence %d: negative count", slots.at(i));
        first[i + 1] = first[i] + counts[i];
        return (int)SVO_OK;
    });
    if (rc) return rc;
    const int64_t total = first[slots.n];
    if (total > (1 << 24)) return svo_set_error(SVO_ERR_INVALID, "svo_submit_pose_updates: %lld samples in one call", (long long)total);
    if (total > 0 && !samples) return svo_set_error(SVO_ERR_INVALID, "svo_submit_pose_updates: no samples");
    for (int64_t k = 0; k < total; k++)
        if (samples[k].flags & ~(uint32_t)SVO_POSE_SAMPLE_CHAIN)
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_pose_updates: sample %lld: unknown flag bits 0x%x", (long long)k, samples[k].flags);
    if (c->failed.load()) return reject_failed(c, "svo_submit_pose_updates");
    submit_shares<svo_ctx::PoseUpdates>(c, slots, [&](svo_ctx::PoseUpdates& u, int i, int) {
        if (counts[i] == 0) return false;                    // (a slot without samples is not in the job)
        u.counts.push_back(counts[i]);
        u.samples.insert(u.samples.end(), samples + first[i], samples + first[i + 1]);
        u.filtered.push_back(filtered ? filtered + first[i] * 6 : nullptr);
        return true;
    }, nothing_more);
    return SVO_OK;
}

extern "C" int svo_update_poses(svo_ctx* c, const int* seqs, const int* counts, int n, const svo_pose_sample* samples,
                                float* filtered) {
    return then_wait(c, svo_submit_pose_updates(c, seqs, counts, n, samples, filtered));
}
