// gains.hip -- kpilqr_download_gains_f32[_partial] and the gain downloads of kpilqr_iterate_streamed2's chunks: the device side of
// downloading the feedback gains K as FP32, and of gathering the gains of a list of trajectories straight into pinned host memory.
//
// K is the largest item a re-linearising host moves per iteration (T*n*m*8 bytes per trajectory, every iteration, for every active
// trajectory: DESIGN.md section 7), and it only ever multiplies the small feedback term x - x_old.  k_gains_f32 gathers the listed
// trajectories' K from the resident FP64 buffer and rounds it into ONE compact float buffer the context owns, which then crosses the
// link with one copy: half the bytes.  The FP64 buffer is only read.
//
// A pure stream (8 bytes in, 4 out per element; no LDS, no atomics).  A trajectory's element count T*n*m is even (n = 2*dof) but not
// generally a multiple of four (Panda, T = 17: 1666), so the unit of work is a PAIR: one 16-byte load and one 8-byte store, both
// aligned for every trajectory -- the source row starts at b*per*8 bytes and the compact destination row at i*per*4 bytes behind a
// hipMalloc base, per even -- and a row has no tail.  Nothing wider is used: it would need a head / tail story for both sides.
//
// The conversion is the C cast (float): IEEE round-to-nearest-even, results in the FP32 subnormal range produced and not flushed (the
// Makefile pins the FP32 denormal mode for this file), magnitudes above FLT_MAX to +-inf, NaN stays NaN.
#include "common.h"

namespace kpilqr {

#define KPG_THREADS 256
#define KPG_ITERS 8                                   // pairs a lane converts per slice: a block's slice is 32 KB in, 16 KB out

// The conversion of a pair, shared by k_gains_f32 and the chunk pipeline's k_gains_out: the one place K is rounded
__device__ __forceinline__ float2 gains_pair_f32(const double2 v) { return make_float2((float)v.x, (float)v.y); }

// Block (x, y): slices x, x + gridDim.x, ... of list rows y, y + gridDim.y, ...; row i is trajectory traj[i] (traj == nullptr: i, the
// whole batch).  pairs = T*n*m / 2.  Every offset is uniform over the block, lanes convert consecutive pairs.
__global__ void __launch_bounds__(KPG_THREADS)
k_gains_f32(int count, const int *__restrict__ traj, long long pairs, const double2 *__restrict__ K, float2 *__restrict__ out)
{
    constexpr long long slice = (long long)KPG_THREADS * KPG_ITERS;
    for (int i = blockIdx.y; i < count; i += gridDim.y) {
        const long long b = traj ? traj[i] : i;
        const double2 *s = K + b * pairs;
        float2 *d = out + (long long)i * pairs;
        for (long long at = (long long)blockIdx.x * slice; at < pairs; at += (long long)gridDim.x * slice) {
            const long long end = at + slice < pairs ? at + slice : pairs;
#pragma unroll KPG_ITERS
            for (long long p = at + threadIdx.x; p < end; p += KPG_THREADS) {
                const double2 v = s[p];
                d[p] = gains_pair_f32(v);
            }
        }
    }
}

// K of `count` trajectories (traj_dev: their indices on the device, or nullptr for trajectories 0 .. count-1) -> out [count][T][n][m] floats
hipError_t launch_gains_f32(Ctx *c, const int *traj_dev, int count, float *out)
{
    const long long pairs = (long long)c->d.T * c->n * c->d.m / 2;
    if (count <= 0 || pairs == 0) return hipSuccess;
    constexpr long long slice = (long long)KPG_THREADS * KPG_ITERS;
    const long long want = (pairs + slice - 1) / slice;
    const dim3 grid((unsigned)(want > 4096 ? 4096 : want), count < 65535 ? count : 65535);
    hipLaunchKernelGGL(k_gains_f32, grid, dim3(KPG_THREADS), 0, c->stream, count, traj_dev, pairs, (const double2 *)(const double *)c->K,
                       (float2 *)out);
    return hipGetLastError();
}

// ---- the chunks of kpilqr_iterate_streamed2: gather, round when asked, store into the caller's pinned buffer ----------------------------
// One kernel family for the three outputs a chunk may owe: K as FP32 (double2 in, float2 out), K of a list as it is (double2), k of a
// list (8-byte elements: a k row has T*m elements, which may be odd, so every second row is off 16-byte alignment on BOTH sides and
// nothing wider than the element is assumed).  Row i of `count` is trajectory traj[i] (traj == nullptr: first + i) of src, `units`
// units long; it goes to row i of dst, compact, in mapped pinned host memory: no staging buffer, no second DMA.  For K the unit is the
// pair, as above: source rows 16-byte and float rows 8-byte aligned, no tail.
// Launch shape of k_copy_out (32 workgroups of 256: they saturate the link and leave the chip to the sweeps of the other chunks).
// The work is cut into slices of KPG_THREADS * KPG_ITERS units that never cross a row; block x takes slices x, x + gridDim.x, ...
// of the launch as a whole, so rows shorter or longer than a round of the grid balance alike, and every offset is uniform over a block.
__device__ __forceinline__ void gains_store(float2 *d, const double2 v) { *d = gains_pair_f32(v); }
__device__ __forceinline__ void gains_store(double2 *d, const double2 v) { *d = v; }
__device__ __forceinline__ void gains_store(double *d, const double v) { *d = v; }

template <class S, class D>
__global__ void __launch_bounds__(KPG_THREADS)
k_gains_out(int count, const int *__restrict__ traj, int first, long long units, const S *__restrict__ src, D *__restrict__ dst)
{
    constexpr long long slice = (long long)KPG_THREADS * KPG_ITERS;
    const long long per_row = (units + slice - 1) / slice, total = per_row * count;
    for (long long g = blockIdx.x; g < total; g += gridDim.x) {
        const long long i = g / per_row, at = (g - i * per_row) * slice;
        const long long b = traj ? traj[i] : first + i;
        const S *s = src + b * units;
        D *d = dst + i * units;
        const long long end = at + slice < units ? at + slice : units;
#pragma unroll KPG_ITERS
        for (long long p = at + threadIdx.x; p < end; p += KPG_THREADS) gains_store(d + p, s[p]);
    }
}

hipError_t launch_gains_out(const Ctx *c, hipStream_t s, GainsForm form, const int *traj, int first, int count, void *dst_host)
{
    const long long perK = (long long)c->d.T * c->n * c->d.m, perk = (long long)c->d.T * c->d.m;
    if (count <= 0) return hipSuccess;
    const dim3 grid(32), block(KPG_THREADS);
    switch (form) {
    case GainsForm::K_f32:
        hipLaunchKernelGGL((k_gains_out<double2, float2>), grid, block, 0, s, count, traj, first, perK / 2, (const double2 *)(const double *)c->K, (float2 *)dst_host);
        break;
    case GainsForm::K_f64:
        hipLaunchKernelGGL((k_gains_out<double2, double2>), grid, block, 0, s, count, traj, first, perK / 2, (const double2 *)(const double *)c->K, (double2 *)dst_host);
        break;
    case GainsForm::k_f64:
        hipLaunchKernelGGL((k_gains_out<double, double>), grid, block, 0, s, count, traj, first, perk, (const double *)c->k, (double *)dst_host);
        break;
    }
    return hipGetLastError();
}

}  // namespace kpilqr
