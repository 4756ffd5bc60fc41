// kp_partial.hip -- kpilqr_update_keypoints: the device side of replacing the key-point lists of SOME trajectories.
//
// A payload laid out by CSR entry (the key-point ordered FD slab, the column store of a column payload) has to follow the lists: new
// lists of one trajectory shift the entry offsets of every later one.  The records of the trajectories that keep their lists are
// already on the device; these two kernels move them -- and the lists themselves -- to their new offsets at HBM rate instead of
// sending them over the link again:
//   k_relocate_entries   old payload buffer -> second buffer, the ranges of the kept trajectories (the others arrive by upload)
//   k_merge_kp_times     old kp_times + the uploaded new lists -> second kp_times buffer
// Both are pure streams (the HBM-bound column).  Never in place: ranges move both ways and may overlap their
// own destination; the context swaps the two buffers afterwards (kpilqr_api.cpp).
#include "common.h"

namespace kpilqr {

#define KPP_THREADS 256
#define KPP_ITERS 16                                  // 16-byte units a lane moves per slice: a block's slice is 64 KB

// first_old / first_new [batch+1]: first entry of every trajectory before and after; upl_first [batch+1]: -1 for a kept trajectory.
// A record is `units` 16-byte units in both payload kinds ((6n+2)*8 and 3n*8 bytes, n even).  Block (x, y): slices x, x + gridDim.x,
// ... of trajectories y, y + gridDim.y, ...; every offset is uniform over the block, lanes move consecutive units.
__global__ void __launch_bounds__(KPP_THREADS)
k_relocate_entries(int batch, int units, const int *__restrict__ first_old, const int *__restrict__ first_new,
                   const int *__restrict__ upl_first, const double2 *__restrict__ src, double2 *__restrict__ dst)
{
    constexpr long long slice = (long long)KPP_THREADS * KPP_ITERS;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        if (upl_first[b] >= 0) continue;                                   // listed: its records come by upload
        const long long len = (long long)(first_old[b + 1] - first_old[b]) * units;
        const double2 *s = src + (long long)first_old[b] * units;
        double2 *d = dst + (long long)first_new[b] * units;
        for (long long at = (long long)blockIdx.x * slice; at < len; at += (long long)gridDim.x * slice) {
            const long long end = at + slice < len ? at + slice : len;
            for (long long i = at + threadIdx.x; i < end; i += KPP_THREADS) d[i] = s[i];
        }
    }
}

// the same walk for the lists: a kept trajectory's times come from the old array, a listed one's from the uploaded lists
__global__ void __launch_bounds__(KPP_THREADS)
k_merge_kp_times(int batch, const int *__restrict__ first_old, const int *__restrict__ first_new, const int *__restrict__ upl_first,
                 const int *__restrict__ old_times, const int *__restrict__ upl_times, int *__restrict__ times)
{
    constexpr int slice = KPP_THREADS * KPP_ITERS;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const int len = first_new[b + 1] - first_new[b];
        const int u = upl_first[b];
        const int *s = u >= 0 ? upl_times + u : old_times + first_old[b];
        int *d = times + first_new[b];
        for (int at = blockIdx.x * slice; at < len; at += gridDim.x * slice) {
            const int end = at + slice < len ? at + slice : len;
            for (int i = at + threadIdx.x; i < end; i += KPP_THREADS) d[i] = s[i];
        }
    }
}

// blocks along x for ranges of at most `longest` elements, slices of `per` each (further slices: the kernels' stride loops)
static unsigned slices(long long longest, long long per)
{
    const long long want = (longest + per - 1) / per;
    return (unsigned)(want < 1 ? 1 : want > 4096 ? 4096 : want);
}

hipError_t launch_relocate_entries(Ctx *c, int units, long long longest_kept_entries, const int *first_old, const int *first_new,
                                   const int *upl_first, const void *src, void *dst)
{
    if (c->d.batch == 0 || longest_kept_entries == 0) return hipSuccess;      // nothing kept, or nothing in it
    const dim3 grid(slices(longest_kept_entries * units, (long long)KPP_THREADS * KPP_ITERS), c->d.batch < 65535 ? c->d.batch : 65535);
    hipLaunchKernelGGL(k_relocate_entries, grid, dim3(KPP_THREADS), 0, c->stream, c->d.batch, units, first_old, first_new, upl_first,
                       (const double2 *)src, (double2 *)dst);
    return hipGetLastError();
}

hipError_t launch_merge_kp_times(Ctx *c, int longest_entries, const int *first_old, const int *first_new, const int *upl_first,
                                 const int *old_times, const int *upl_times, int *times)
{
    if (c->d.batch == 0 || longest_entries == 0) return hipSuccess;
    const dim3 grid(slices(longest_entries, (long long)KPP_THREADS * KPP_ITERS), c->d.batch < 65535 ? c->d.batch : 65535);
    hipLaunchKernelGGL(k_merge_kp_times, grid, dim3(KPP_THREADS), 0, c->stream, c->d.batch, first_old, first_new, upl_first, old_times,
                       upl_times, times);
    return hipGetLastError();
}

}  // namespace kpilqr
