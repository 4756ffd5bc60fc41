// kp_merge.h -- the host arithmetic of kpilqr_update_keypoints and the calls on a subset of the batch: checks of per-DoF key-point
// lists, their per-trajectory flags, the walk over a subset's runs of adjacent trajectories, and the merge of a subset's new lists
// into the batch CSR.  Plain C++ without HIP on purpose: kpilqr_api.cpp uses it, and a stand-alone program can drive it under the
// host sanitizers (tools/kp_merge_fuzz.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace kpilqr {

// what the host knows about ONE trajectory's lists (Ctx::kp_flags_host); the context's flags are the AND over the batch
enum : unsigned char {
    kKpCanonical = 1,      // every DoF list strictly increasing, first 0, last T-1 (what the fused sweeps walk)
    kKpUniform = 2,        // all DoFs share one list (set_interval)
};

// kpilqr_set_keypoints' checks of `nlists` lists: offsets from 0 and monotone, times in [0, T).  nullptr: fine, else the message.
inline const char *kp_check_lists(size_t nlists, int T, const int *offs, const int *times)
{
    if (offs[0] != 0 || offs[nlists] < 0) return "kp_offsets must start at 0";
    for (size_t i = 0; i < nlists; i++)
        if (offs[i + 1] < offs[i]) return "kp_offsets not monotone";
    for (int i = 0; i < offs[nlists]; i++)
        if (times[i] < 0 || times[i] >= T) return "kp_times out of [0,T)";
    return nullptr;
}

// flags of one trajectory: offs [dof+1] are its offsets INTO times
inline unsigned char kp_traj_flags(int dof, int T, const int *offs, const int *times)
{
    unsigned char f = kKpCanonical | kKpUniform;
    for (int i = 0; i < dof && (f & kKpCanonical); i++) {
        const int a = offs[i], e = offs[i + 1];
        if (e <= a || times[a] != 0 || times[e - 1] != T - 1) { f &= (unsigned char)~kKpCanonical; break; }
        for (int j = a + 1; j < e; j++) if (times[j] <= times[j - 1]) { f &= (unsigned char)~kKpCanonical; break; }
    }
    const int len0 = offs[1] - offs[0];
    for (int i = 1; i < dof; i++)
        if (offs[i + 1] - offs[i] != len0 || (len0 > 0 && memcmp(times + offs[i], times + offs[0], sizeof(int) * (size_t)len0) != 0)) { f &= (unsigned char)~kKpUniform; break; }
    return f;
}

inline unsigned char kp_batch_flags(int batch, const unsigned char *flags)
{
    unsigned char f = kKpCanonical | kKpUniform;
    for (int b = 0; b < batch; b++) f &= flags[b];
    return f;
}

// `traj` strictly increasing and within [0, batch)
inline bool kp_traj_list_ok(int batch, int count, const int *traj)
{
    for (int i = 0; i < count; i++)
        if (traj[i] < 0 || traj[i] >= batch || (i > 0 && traj[i] <= traj[i - 1])) return false;
    return true;
}

// f(i, first, len) for every maximal run traj[i] .. traj[i + len - 1] = first .. first + len - 1 of adjacent trajectories in a
// strictly increasing list, in order (the calls on a subset copy or launch once per run).  Stops at the first non-zero result of f
// and returns it; 0: every run was visited.
template <class F>
inline int kp_for_each_run(int count, const int *traj, F f)
{
    for (int i = 0; i < count;) {
        int j = i;
        while (j + 1 < count && traj[j + 1] == traj[j] + 1) j++;
        if (const int rc = f(i, traj[i], j - i + 1)) return rc;
        i = j + 1;
    }
    return 0;
}

// kpilqr_generate_keypoints_partial: the counts [nlists] the placement kernel wrote for the listed trajectories' DoF lists, compact
// -> offs [nlists + 1] from 0, the new lists' own CSR (what kp_merge_offsets takes as new_offs).  0: done | 1: a count outside
// [0, T], which is not something the kernel writes | 2: more entries than an int counts.  offs is not to be used unless 0.
inline int kp_offsets_from_counts(size_t nlists, int T, const int *counts, int *offs)
{
    int64_t at = 0;
    for (size_t i = 0; i < nlists; i++) {
        if (counts[i] < 0 || counts[i] > T) return 1;
        offs[i] = (int)at;
        at += counts[i];
        if (at > INT32_MAX) return 2;
    }
    offs[nlists] = (int)at;
    return 0;
}

// The batch CSR with the lists of the `count` trajectories in `traj` replaced: new_offs [count*dof+1] (from 0) are theirs, old_offs
// [batch*dof+1] everybody's so far.  Writes merged [batch*dof+1] and, per trajectory, its first entry before (old_first [batch+1])
// and after (new_first [batch+1]) and where its times come from: upl_first [batch+1] = first entry inside the new lists' times for
// a listed trajectory, -1 for a kept one (whose records move from old_first[b] to new_first[b]; a kept range keeps its length).
// false: the merged total does not fit an int (nothing the caller may use has been written).
inline bool kp_merge_offsets(int batch, int dof, const int *old_offs, int count, const int *traj, const int *new_offs, int *merged,
                             int *old_first, int *new_first, int *upl_first)
{
    int64_t total = old_offs[(size_t)batch * dof];
    for (int i = 0; i < count; i++) {
        const size_t o = (size_t)traj[i] * dof;
        total += (int64_t)(new_offs[(size_t)(i + 1) * dof] - new_offs[(size_t)i * dof]) - (old_offs[o + dof] - old_offs[o]);
    }
    if (total > INT32_MAX) return false;
    int at = 0, li = 0;
    for (int b = 0; b < batch; b++) {
        const bool listed = li < count && traj[li] == b;
        const int *src = listed ? new_offs + (size_t)li * dof : old_offs + (size_t)b * dof;
        old_first[b] = old_offs[(size_t)b * dof];
        new_first[b] = at;
        upl_first[b] = listed ? src[0] : -1;
        for (int i = 0; i < dof; i++) { merged[(size_t)b * dof + i] = at; at += src[i + 1] - src[i]; }
        if (listed) li++;
    }
    merged[(size_t)batch * dof] = at;
    old_first[batch] = old_offs[(size_t)batch * dof];
    new_first[batch] = at;
    upl_first[batch] = -1;
    return true;
}

}  // namespace kpilqr
