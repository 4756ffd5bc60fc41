// rows_in.hip -- kpilqr_iterate_streamed4 with upload_traj: the device side of uploading the inputs of a LIST of trajectories inside
// the chunks of a streamed iteration.
//
// A chunk's share of a compact input (the listed trajectories' rows back to back) crosses the link with ONE copy into a staging
// region of the context; k_rows_in then moves the rows device-to-device from staging to their trajectories' places.  One copy per
// run of adjacent trajectories -- what the explicit partial calls do -- would be a DMA submission per few microseconds of link time
// here (a scattered half of 1024 trajectories: over a thousand per iteration), and a kernel that reads pinned memory itself loses
// to the SDMA-up / kernel-down pairing of the pipeline (profiles/r02_pcie_inclusive.txt).
//
// Two row forms:
//   fixed     r, r_x, r_u, u_nom: every row has `units` 8-byte elements.  A row may hold an odd number of doubles (Panda, T = 17:
//             u_nom rows of 119), so every second row is off 16-byte alignment on both sides and nothing wider than the element is
//             assumed -- as k_gains_out (gains.hip) treats k.  Row i of the slice sits at staging + i*units and goes to
//             dst + traj[i]*units.
//   by entry  the key-point ordered records and the FP64 key-point columns: the row of trajectory b is its CSR entry range
//             [kp_offsets[b*dof], kp_offsets[(b+1)*dof]) of the lists the context holds on the device, `upe` 16-byte units per
//             entry (records: (6n+2)/2, columns: 3n/2; both whole because n is even, and every range starts 16-byte aligned behind
//             the hipMalloc bases).  Its source is entry src_first[b] of the staging region: the running sum over the chunk's slice
//             of the list, which the host, knowing the lists, has put beside the list.
// A pure copy (no LDS, no atomics, no arithmetic): launch shape and slice scheme of k_gains_out -- 32 workgroups of 256, slices of
// KPR_THREADS * KPR_ITERS units that never cross a row, every offset uniform over a block, lanes on consecutive units.
// The FP32 columns do not come here: columns_f32.hip decodes them from their staging buffer straight into the listed ranges.
#include "common.h"

namespace kpilqr {

#define KPR_THREADS 256
#define KPR_ITERS 8

// fixed rows: the work is count * ceil(units / slice) slices; block x takes slices x, x + gridDim.x, ... of the launch as a whole
__global__ void __launch_bounds__(KPR_THREADS)
k_rows_in(int count, const int *__restrict__ traj, long long units, const double *__restrict__ src, double *__restrict__ dst)
{
    constexpr long long slice = (long long)KPR_THREADS * KPR_ITERS;
    const long long per_row = (units + slice - 1) / slice, total = per_row * count;
    for (long long g = blockIdx.x; g < total; g += gridDim.x) {
        const long long i = g / per_row, at = (g - i * per_row) * slice;
        const long long b = traj[i];
        const double *s = src + i * units;
        double *d = dst + b * units;
        const long long end = at + slice < units ? at + slice : units;
#pragma unroll KPR_ITERS
        for (long long p = at + threadIdx.x; p < end; p += KPR_THREADS) d[p] = s[p];
    }
}

// rows by entry: rows differ in length, so every block walks the rows and takes, of row i, the slices (x - i) mod gridDim.x,
// + gridDim.x, ...: rows of one slice (a short list) spread over the blocks as rows of many do
__global__ void __launch_bounds__(KPR_THREADS)
k_rows_in_entries(int count, const int *__restrict__ traj, int dof, long long upe, const int *__restrict__ kp_offsets,
                  const int *__restrict__ src_first, const double2 *__restrict__ src, double2 *__restrict__ dst)
{
    constexpr long long slice = (long long)KPR_THREADS * KPR_ITERS;
    const int G = (int)gridDim.x;
    for (int i = 0; i < count; i++) {
        const int b = traj[i];
        const int e0 = kp_offsets[(long long)b * dof];
        const long long units = (long long)(kp_offsets[(long long)(b + 1) * dof] - e0) * upe;
        const double2 *s = src + (long long)src_first[b] * upe;
        double2 *d = dst + (long long)e0 * upe;
        const int x = (int)(((long long)blockIdx.x + G - i % G) % G);
        for (long long at = x * slice; at < units; at += G * slice) {
            const long long end = at + slice < units ? at + slice : units;
#pragma unroll KPR_ITERS
            for (long long p = at + threadIdx.x; p < end; p += KPR_THREADS) d[p] = s[p];
        }
    }
}

// The mirror image for the listed sweeps (kpilqr_backward_partial, kpilqr_forward_linear_partial): the listed trajectories' rows of a small
// per-trajectory output (status: one int; delta_J: one double; cost_pred: n_alpha doubles) gathered into a compact staging array that
// leaves with ONE copy, however scattered the list is.  Rows of a few 4-byte words: one thread per word, a pure copy.
// (A chunk of kpilqr_iterate_streamed5 hands it its slice of the caller's mapped pinned array for dst: plain stores through the pointer.)
__global__ void __launch_bounds__(KPR_THREADS)
k_rows_out(int count, const int *__restrict__ traj, int words, const unsigned *__restrict__ src, unsigned *__restrict__ dst)
{
    const long long total = (long long)count * words;
    for (long long g = (long long)blockIdx.x * KPR_THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * KPR_THREADS) {
        const long long i = g / words, p = g - i * words;
        dst[g] = src[(long long)traj[i] * words + p];
    }
}

hipError_t launch_rows_out(hipStream_t s, const int *traj_dev, int count, int words, const void *src, void *staging)
{
    if (count <= 0 || words <= 0) return hipSuccess;
    const long long total = (long long)count * words;
    const int blocks = (int)((total + KPR_THREADS - 1) / KPR_THREADS < 32 ? (total + KPR_THREADS - 1) / KPR_THREADS : 32);
    hipLaunchKernelGGL(k_rows_out, dim3(blocks), dim3(KPR_THREADS), 0, s, count, traj_dev, words, (const unsigned *)src, (unsigned *)staging);
    return hipGetLastError();
}

// `count` rows of `units` doubles: row i of `staging` (device) -> row traj[i] (traj on the device) of dst, on stream s
hipError_t launch_rows_in(hipStream_t s, const int *traj_dev, int count, long long units, const double *staging, double *dst)
{
    if (count <= 0 || units <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rows_in, dim3(32), dim3(KPR_THREADS), 0, s, count, traj_dev, units, staging, dst);
    return hipGetLastError();
}

// The entry ranges of `count` trajectories traj[i] (device) of the CONTEXT's device CSR (c is never a view), rec_bytes per entry (a
// multiple of 16): from entry src_first[traj[i]] of `staging` (src_first [batch] on the device) to the trajectory's own range of dst
hipError_t launch_rows_in_entries(const Ctx *c, hipStream_t s, const int *traj_dev, int count, const int *src_first_dev, size_t rec_bytes,
                                  const void *staging, void *dst)
{
    if (count <= 0 || rec_bytes == 0) return hipSuccess;
    if ((rec_bytes & 15) || (((size_t)staging | (size_t)dst) & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rows_in_entries, dim3(32), dim3(KPR_THREADS), 0, s, count, traj_dev, c->d.dof, (long long)(rec_bytes / 16),
                       (const int *)c->kp_offsets, src_first_dev, (const double2 *)staging, (double2 *)dst);
    return hipGetLastError();
}

}  // namespace kpilqr
