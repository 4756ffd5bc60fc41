// kp_merge_fuzz.cpp -- the host arithmetic of kpilqr_update_keypoints (trajoptkp_amd/csrc/kp_merge.h) on random CSR moves, as a
// stand-alone program for the host sanitizers:
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/kp_merge_fuzz.cpp -o kp_merge_fuzz && ./kp_merge_fuzz
// Random batches of per-DoF lists (canonical, broken, uniform, empty), a random strictly increasing subset with new lists of other
// lengths: the merged offsets, the move table and the per-trajectory flags are held against a restatement with std::vector, and
// the move itself is replayed on byte buffers -- what k_relocate_entries / k_merge_kp_times do with the same three arrays -- into
// allocations of exactly the needed size, so that an index one past a range is a sanitizer report.  The walk over runs of adjacent
// trajectories (kp_for_each_run: what every call on a subset copies or launches by) is held against a naive restatement on random
// strictly increasing lists, the empty list, one element, all adjacent and none adjacent included.  The offsets
// kpilqr_generate_keypoints_partial forms from the per-list counts it reads back (kp_offsets_from_counts) are held against the new
// lists' own offsets in every trial, with a count the kernel cannot write and the edge of an int.  Prints the number of trials.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../trajoptkp_amd/csrc/kp_merge.h"

using namespace kpilqr;

struct Lists { std::vector<std::vector<int>> dof; };      // one trajectory

static Lists random_lists(std::mt19937 &rng, int dof, int T)
{
    Lists l;
    const int kind = (int)(rng() % 8);
    std::vector<int> shared;
    for (int i = 0; i < dof; i++) {
        std::vector<int> t;
        if (kind == 0) { /* empty lists */ }
        else if (kind == 1) { for (int j = 0, n = (int)(rng() % 5); j < n; j++) t.push_back((int)(rng() % T)); }       // any order: not canonical
        else {
            t.push_back(0);
            for (int s = 1; s < T - 1; s++) if (rng() % 3 == 0) t.push_back(s);
            t.push_back(T - 1);
        }
        if (kind >= 6) { if (i == 0) shared = t; else t = shared; }       // uniform
        l.dof.push_back(t);
    }
    return l;
}

static void flatten(const std::vector<Lists> &trajs, std::vector<int> &offs, std::vector<int> &times)
{
    offs.assign(1, 0); times.clear();
    for (const Lists &l : trajs)
        for (const std::vector<int> &t : l.dof) { times.insert(times.end(), t.begin(), t.end()); offs.push_back((int)times.size()); }
}

static unsigned char flags_of(const Lists &l, int T)
{
    unsigned char f = kKpCanonical | kKpUniform;
    for (const std::vector<int> &t : l.dof) {
        bool ok = !t.empty() && t.front() == 0 && t.back() == T - 1;
        for (size_t j = 1; ok && j < t.size(); j++) ok = t[j] > t[j - 1];
        if (!ok) f &= (unsigned char)~kKpCanonical;
        if (t != l.dof[0]) f &= (unsigned char)~kKpUniform;
    }
    return f;
}

// kp_for_each_run on `traj` (an exactly sized heap copy) against the definition: the runs partition the list in order, each is a
// stretch of consecutive indices, none could be longer, and i is the position of a run's first element; a non-zero result of f
// stops the walk and comes back.  -> the line of the first failed requirement, 0: fine.
static int run_walk_fails(const std::vector<int> &list)
{
#define RUN_REQUIRE(x) do { if (!(x)) { std::free(traj); return __LINE__; } } while (0)
    const int count = (int)list.size();
    int *traj = (int *)std::malloc(sizeof(int) * list.size() + 1);
    for (int i = 0; i < count; i++) traj[i] = list[i];
    struct Run { int i, first, len; };
    std::vector<Run> runs;
    RUN_REQUIRE(kp_for_each_run(count, traj, [&](int i, int first, int len) { runs.push_back({i, first, len}); return 0; }) == 0);
    int at = 0;                                                            // position in the list the next run has to start at
    for (size_t r = 0; r < runs.size(); r++) {
        RUN_REQUIRE(runs[r].i == at && runs[r].len >= 1 && at + runs[r].len <= count && runs[r].first == list[at]);
        for (int j = 0; j < runs[r].len; j++) RUN_REQUIRE(list[at + j] == runs[r].first + j);
        at += runs[r].len;
        RUN_REQUIRE(at == count || list[at] != list[at - 1] + 1);          // maximal
    }
    RUN_REQUIRE(at == count);
    size_t naive = 0;                                                      // runs = 1 + places where the list jumps
    for (int i = 0; i < count; i++) naive += i == 0 || list[i] != list[i - 1] + 1;
    RUN_REQUIRE(runs.size() == naive);
    for (size_t stop = 0; stop < runs.size(); stop++) {                    // the first non-zero result ends the walk
        size_t calls = 0;
        RUN_REQUIRE(kp_for_each_run(count, traj, [&](int, int, int) { return calls++ == stop ? 7 + (int)stop : 0; }) == 7 + (int)stop);
        RUN_REQUIRE(calls == stop + 1);
    }
    std::free(traj);
    return 0;
#undef RUN_REQUIRE
}

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "trial %d: %s failed (line %d)\n", trial, #x, __LINE__); return 1; } } while (0)

int main()
{
    std::mt19937 rng(20240611);
    int trial = 0;
    for (; trial < 600; trial++) {
        const int B = 1 + (int)(rng() % 9), dof = 1 + (int)(rng() % 4), T = 2 + (int)(rng() % 12), unit = 1 + (int)(rng() % 5);
        std::vector<Lists> old_t(B);
        for (Lists &l : old_t) l = random_lists(rng, dof, T);
        std::vector<int> traj;
        for (int b = 0; b < B; b++) if (rng() % 3 == 0 || trial % 11 == 0) traj.push_back(b);
        if (trial % 13 == 0) traj.clear();
        std::vector<Lists> upd, want = old_t;
        for (int b : traj) { upd.push_back(random_lists(rng, dof, T)); want[b] = upd.back(); }

        std::vector<int> old_offs, old_times, new_offs, new_times, want_offs, want_times;
        flatten(old_t, old_offs, old_times); flatten(upd, new_offs, new_times); flatten(want, want_offs, want_times);
        REQUIRE(kp_check_lists((size_t)B * dof, T, old_offs.data(), old_times.data()) == nullptr);
        REQUIRE(kp_check_lists(traj.size() * dof, T, new_offs.data(), new_times.data()) == nullptr);
        REQUIRE(kp_traj_list_ok(B, (int)traj.size(), traj.data()));
        REQUIRE(run_walk_fails(traj) == 0);

        // kpilqr_generate_keypoints_partial: the new lists' offsets from the per-list counts the device reports (exactly sized arrays)
        {
            const size_t nnew = traj.size() * dof;
            int *counts = (int *)std::malloc(sizeof(int) * nnew + 1), *offs = (int *)std::malloc(sizeof(int) * (nnew + 1));
            bool fits = true;                                               // (a list in any order may repeat a time: more than T entries)
            for (size_t i = 0; i < nnew; i++) { counts[i] = new_offs[i + 1] - new_offs[i]; fits = fits && counts[i] <= T; }
            REQUIRE(kp_offsets_from_counts(nnew, T, counts, offs) == (fits ? 0 : 1));
            for (size_t i = 0; fits && i <= nnew; i++) REQUIRE(offs[i] == new_offs[i]);
            if (nnew && fits) {                                                     // a count the kernel cannot have written
                const size_t at = rng() % nnew;
                const int was = counts[at];
                counts[at] = rng() % 2 ? -1 : T + 1;
                REQUIRE(kp_offsets_from_counts(nnew, T, counts, offs) == 1);
                counts[at] = was;
            }
            std::free(counts); std::free(offs);
        }

        // exactly sized heap arrays: one element too far is a report
        int *merged =(int *)std::malloc(sizeof(int) * ((size_t)B * dof + 1)), *mv = (int *)std::malloc(sizeof(int) * 3 * ((size_t)B + 1));
        int *first_old = mv, *first_new = mv + B + 1, *upl_first = mv + 2 * (B + 1);
        REQUIRE(kp_merge_offsets(B, dof, old_offs.data(), (int)traj.size(), traj.data(), new_offs.data(), merged, first_old, first_new, upl_first));
        for (size_t i = 0; i < want_offs.size(); i++) REQUIRE(merged[i] == want_offs[i]);

        // the lists and the records, moved as the kernels move them
        const int total_old = old_offs.back(), total_new = want_offs.back();
        unsigned char *rec_old = (unsigned char *)std::malloc((size_t)total_old * unit + 1), *rec_new = (unsigned char *)std::malloc((size_t)total_new * unit + 1);
        int *times = (int *)std::malloc(sizeof(int) * ((size_t)total_new + 1));
        for (int i = 0; i < total_old * unit; i++) rec_old[i] = (unsigned char)rng();
        for (int i = 0; i < total_new * unit; i++) rec_new[i] = 0xEE;
        for (int b = 0; b < B; b++) {
            const int len = first_new[b + 1] - first_new[b];
            const int *src = upl_first[b] >= 0 ? new_times.data() + upl_first[b] : old_times.data() + first_old[b];
            for (int i = 0; i < len; i++) times[first_new[b] + i] = src[i];
            if (upl_first[b] >= 0) continue;
            REQUIRE(first_old[b + 1] - first_old[b] == len);               // a kept range keeps its length
            for (int i = 0; i < len * unit; i++) rec_new[(size_t)first_new[b] * unit + i] = rec_old[(size_t)first_old[b] * unit + i];
        }
        for (int i = 0; i < total_new; i++) REQUIRE(times[i] == want_times[i]);
        size_t li = 0;
        for (int b = 0; b < B; b++) {
            const bool listed = li < traj.size() && traj[li] == b;
            REQUIRE((upl_first[b] >= 0) == listed);
            const int o = old_offs[(size_t)b * dof], w = want_offs[(size_t)b * dof], len = want_offs[(size_t)(b + 1) * dof] - w;
            for (int i = 0; i < len * unit; i++)
                REQUIRE(rec_new[(size_t)w * unit + i] == (listed ? 0xEE : rec_old[(size_t)o * unit + i]));
            if (listed) li++;
        }

        // flags: per trajectory from its own offsets, the batch's as the AND
        std::vector<unsigned char> flags(B);
        for (int b = 0; b < B; b++) flags[b] = kp_traj_flags(dof, T, old_offs.data() + (size_t)b * dof, old_times.data());
        for (size_t i = 0; i < traj.size(); i++) flags[traj[i]] = kp_traj_flags(dof, T, new_offs.data() + i * dof, new_times.data());
        unsigned char all = kKpCanonical | kKpUniform;
        for (int b = 0; b < B; b++) { REQUIRE(flags[b] == flags_of(want[b], T)); all &= flags_of(want[b], T); }
        REQUIRE(kp_batch_flags(B, flags.data()) == all);

        // what the ABI refuses
        if (!traj.empty()) {
            std::vector<int> bad = traj;
            bad.push_back(traj.back());                                     // not strictly increasing
            REQUIRE(!kp_traj_list_ok(B, (int)bad.size(), bad.data()));
            bad = traj; bad[0] = B;
            REQUIRE(!kp_traj_list_ok(B, (int)bad.size(), bad.data()));
            if (!new_times.empty()) {
                std::vector<int> t2 = new_times; t2[rng() % t2.size()] = T;
                REQUIRE(kp_check_lists(traj.size() * dof, T, new_offs.data(), t2.data()) != nullptr);
            }
        }
        std::free(merged); std::free(mv); std::free(rec_old); std::free(rec_new); std::free(times);
    }
    // the run walk on longer lists: every density from none adjacent to all adjacent, and the corner cases by hand
    int walks = 0;
    for (; walks < 2000; walks++) {
        const int B = 1 + (int)(rng() % 40), keep = (int)(rng() % 11);      // keep / 10: the chance that an index is listed
        std::vector<int> traj;
        for (int b = 0; b < B; b++) if ((int)(rng() % 10) < keep) traj.push_back(b);
        REQUIRE(kp_traj_list_ok(B, (int)traj.size(), traj.data()) && run_walk_fails(traj) == 0);
    }
    const std::vector<int> corner[] = {{}, {0}, {5}, {0, 1, 2, 3, 4}, {3, 4, 5}, {0, 2, 4, 6}, {1, 3}, {0, 1, 3, 4, 5, 9}, {0, 2, 3}};
    for (const std::vector<int> &traj : corner) { REQUIRE(run_walk_fails(traj) == 0); walks++; }
    // counts -> offsets at the edge of an int: the largest total that fits, and one entry more (the sum is formed in 64 bits)
    {
        const int T = INT32_MAX / 4 + 1;                                    // 4 T = 2^31 > INT32_MAX >= 4 T - 1
        int counts[4] = {T, T, T, T - 1}, offs[5];
        REQUIRE(kp_offsets_from_counts(4, T, counts, offs) == 0 && offs[4] == INT32_MAX && offs[3] == 3 * (int64_t)T);
        counts[3] = T;
        REQUIRE(kp_offsets_from_counts(4, T, counts, offs) == 2);
        REQUIRE(kp_offsets_from_counts(0, T, counts, offs) == 0 && offs[0] == 0);
    }
    std::printf("kp_merge_fuzz: %d trials ok, %d run walks ok\n", trial, walks);
    return 0;
}
