// residuals_f32.hip -- kpilqr_upload_residual_jacobians_f32[_partial]: the device side of uploading the per-step residual Jacobians
// r_x [batch][T+1][nr][n] and r_u [batch][T+1][nr][m] as FP32 -- and, below, of taking them inside the chunks of kpilqr_iterate_streamed6.
//
// They are the largest upload of a host whose residuals are not affine in the state (7.06 MB per trajectory
// at the headline shape, every linearisation).  The caller sends a plain (float) cast of them -- r_x has no unit entry that would eat
// the mantissa, so nothing is encoded (include/kpilqr.h) -- into a staging buffer the context owns, and k_widen_rows widens them into
// the FP64 buffers the sweeps read:
//     dst[(traj ? traj[i] : i) * per + e] = (double)src[i * per + e]        per = (T+1) * nr * cols elements of a trajectory
// an exact widening and nothing else (FP32 subnormals widen to their value; NaN stays NaN, +-inf and -0 stay).  What the buffers then
// hold is what kpilqr_upload_residuals[_partial] would have copied into them from the widened doubles; nothing downstream can tell.
//
// A pure stream (4 bytes in, 8 out per element; no LDS, no atomics).  A block row is a listed trajectory: its rows are one contiguous
// range of the compact source and of the destination, so a scattered list costs no copy per run.  The unit of work is a template flag:
//   PAIR   per is even (r_x always: n = 2 dof): a trajectory's rows start on a pair in both buffers behind their hipMalloc bases,
//          whatever i and traj[i] are: one 8-byte load and one 16-byte store per unit, the widest store there is.
//   !PAIR  per is odd (r_u of acrobot at T = 36: 37 * 5 * 1 = 185): trajectory i of the source and trajectory traj[i] of the
//          destination can sit on different parities, so nothing is assumed beyond the element: a 4-byte load and an 8-byte store.
// Lanes take consecutive units.  Every offset is 64-bit: batch 1024 x T 3000 x 196 elements is 6e8 elements and 4.8e9 bytes.
//
// Compiled with -ffp-contract=off like the other streaming kernels, and with the FP32 denormal mode pinned (the Makefile): a
// subnormal float must widen to its value, not to zero.
#include "common.h"

namespace kpilqr {

#define RJ32_THREADS 256
#define RJ32_ITERS 8                                  // units a lane widens per slice: a block's slice of pairs is 16 KB in, 32 KB out

template <bool PAIR> struct Rj32Unit { using In = float; using Out = double; };
template <> struct Rj32Unit<true> { using In = float2; using Out = double2; };

__device__ __forceinline__ double rj32_widen(float v) { return (double)v; }
__device__ __forceinline__ double2 rj32_widen(float2 v) { return make_double2((double)v.x, (double)v.y); }

// Block (x, y): slices x, x + gridDim.x, ... of rows y, y + gridDim.y, ... of `count` rows.  Row i is trajectory traj[i] (device,
// the context's traj_list) or, traj == nullptr, trajectory i.  units: units per trajectory (per / 2 pairs, or per elements).  The
// trajectory, the slice's offset and its length are uniform over the block.
template <bool PAIR>
__global__ void __launch_bounds__(RJ32_THREADS)
k_widen_rows(int count, long long units, const int *__restrict__ traj, const typename Rj32Unit<PAIR>::In *__restrict__ src,
             typename Rj32Unit<PAIR>::Out *__restrict__ dst)
{
    constexpr int slice = RJ32_THREADS * RJ32_ITERS;
    for (int i = (int)blockIdx.y; i < count; i += gridDim.y) {
        const long long b = traj ? traj[i] : i;
        const auto *s = src + (long long)i * units;
        auto *q = dst + b * units;
        for (long long at = (long long)blockIdx.x * slice; at < units; at += (long long)gridDim.x * slice) {
            const int len = (int)(at + slice < units ? slice : units - at);
            const auto *ss = s + at;
            auto *qs = q + at;
#pragma unroll RJ32_ITERS
            for (int p = threadIdx.x; p < len; p += RJ32_THREADS) qs[p] = rj32_widen(ss[p]);
        }
    }
}

// `count` trajectories of `per` floats each, compact in src (device), widened into rows traj[i] (device list; nullptr: rows 0 ..
// count-1) of dst, `per` doubles per trajectory, on the context's stream.  src is 8-byte aligned when per is even.
hipError_t launch_widen_rows(Ctx *c, const int *traj_dev, int count, long long per, const float *src, double *dst)
{
    if (count <= 0 || per <= 0) return hipSuccess;
    const bool pair = per % 2 == 0;
    const long long units = pair ? per / 2 : per;
    constexpr long long slice = (long long)RJ32_THREADS * RJ32_ITERS;
    // a trajectory's slices are walked by up to 256 blocks (Panda, T = 3000: r_x is 144 slices of pairs), so that one trajectory
    // alone still covers the device
    const long long want = (units + slice - 1) / slice;
    const dim3 grid((unsigned)(want > 256 ? 256 : want), (unsigned)(count < 65535 ? count : 65535));
    if (pair)
        hipLaunchKernelGGL(k_widen_rows<true>, grid, dim3(RJ32_THREADS), 0, c->stream, count, units, traj_dev, (const float2 *)src, (double2 *)dst);
    else
        hipLaunchKernelGGL(k_widen_rows<false>, grid, dim3(RJ32_THREADS), 0, c->stream, count, units, traj_dev, src, dst);
    return hipGetLastError();
}

// ---- the same widening inside the chunks of kpilqr_iterate_streamed6 ----------------------------------------------------------------
// A chunk pays ONE launch for BOTH arrays (the sweeps are latency-bound): two descriptors, and a split of the x range of the grid
// selects the array -- blocks [0, x.blocks) of a block row walk the slices of r_x, the next u.blocks those of r_u.  An array that is
// not given has zero units and zero blocks.  src is row 0 of the launch: the chunk's slice of the staging buffer (uploads by SDMA) or
// of the caller's pinned floats themselves (KPILQR_PIPE_COPY bit 0: no staging buffer, no second pass over HBM); dst is the
// CONTEXT's buffer.
struct Rj32Array {
    const float *src;
    double *dst;
    long long units;              // per trajectory: pairs, or (r_u with an odd element count) elements
    unsigned blocks;
};

// slices bx, bx + nbx, ... of row `row` of the source into trajectory b of the destination
template <bool PAIR>
__device__ __forceinline__ void rj32_widen_row(const Rj32Array &a, long long row, long long b, unsigned bx, unsigned nbx)
{
    constexpr int slice = RJ32_THREADS * RJ32_ITERS;
    const auto *s = (const typename Rj32Unit<PAIR>::In *)a.src + row * a.units;
    auto *q = (typename Rj32Unit<PAIR>::Out *)a.dst + b * a.units;
    for (long long at = (long long)bx * slice; at < a.units; at += (long long)nbx * slice) {
        const int len = (int)(at + slice < a.units ? slice : a.units - at);
        const auto *ss = s + at;
        auto *qs = q + at;
#pragma unroll RJ32_ITERS
        for (int p = threadIdx.x; p < len; p += RJ32_THREADS) qs[p] = rj32_widen(ss[p]);
    }
}

// Block (x, y): rows y, y + gridDim.y, ... of `count` rows.  Row i is trajectory traj[i] (device: the chunk's slice of the upload
// list) or, traj == nullptr, trajectory first + i.  r_x is always on pairs (n = 2 dof); PAIR_U: r_u is too.  The pair path assumes
// 8-byte aligned sources (a trajectory's element count is even there, so every row of an 8-byte aligned array is); the element path
// assumes nothing beyond the float: a chunk's slice of r_u32 can start on an odd one.
template <bool PAIR_U>
__global__ void __launch_bounds__(RJ32_THREADS)
k_widen_jacobians(int count, int first, const int *__restrict__ traj, Rj32Array x, Rj32Array u)
{
    const bool is_x = blockIdx.x < x.blocks;
    for (int i = (int)blockIdx.y; i < count; i += gridDim.y) {
        const long long b = traj ? traj[i] : first + i;
        if (is_x) rj32_widen_row<true>(x, i, b, blockIdx.x, x.blocks);
        else rj32_widen_row<PAIR_U>(u, i, b, blockIdx.x - x.blocks, u.blocks);
    }
}

static Rj32Array rj32_array(const float *src, double *dst, long long per, bool pair)
{
    constexpr long long slice = (long long)RJ32_THREADS * RJ32_ITERS;
    if (!src || per <= 0) return {nullptr, nullptr, 0, 0};
    const long long units = pair ? per / 2 : per, want = (units + slice - 1) / slice;
    return {src, dst, units, (unsigned)(want > 256 ? 256 : want)};          // (up to 256 blocks per trajectory, as above)
}

// `count` rows on stream s: row i of src_x (perx floats, even) and of src_u (peru floats) widened into trajectory traj[i] (device;
// nullptr: first + i) of dst_x / dst_u.  A NULL source is an array that is not given.  src_x, and src_u when peru is even, are 8-byte
// aligned.
hipError_t launch_widen_jacobians(hipStream_t s, const int *traj_dev, int first, int count, long long perx, const float *src_x, double *dst_x,
                                  long long peru, const float *src_u, double *dst_u)
{
    const bool pair_u = peru % 2 == 0;
    const Rj32Array x = rj32_array(src_x, dst_x, perx, true), u = rj32_array(src_u, dst_u, peru, pair_u);
    if (count <= 0 || x.blocks + u.blocks == 0) return hipSuccess;
    const dim3 grid(x.blocks + u.blocks, (unsigned)(count < 65535 ? count : 65535));
    if (pair_u) hipLaunchKernelGGL(k_widen_jacobians<true>, grid, dim3(RJ32_THREADS), 0, s, count, first, traj_dev, x, u);
    else hipLaunchKernelGGL(k_widen_jacobians<false>, grid, dim3(RJ32_THREADS), 0, s, count, first, traj_dev, x, u);
    return hipGetLastError();
}

}  // namespace kpilqr
