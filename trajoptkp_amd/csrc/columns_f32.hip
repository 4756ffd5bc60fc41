// columns_f32.hip -- kpilqr_upload_kp_columns_f32[_partial]: the device side of uploading the key-point columns as FP32.
//
// The columns are the largest upload of a host that differences itself (3n doubles per key-point entry, every iteration: DESIGN.md
// section 7).  The caller sends them as floats -- with the unit entry of A's columns REMOVED before its cast, so that FP32's 24 bits
// go to the O(dt) part and not to the 1 (include/kpilqr.h, profiles/columns_f32.txt) -- into a staging buffer the context owns, and
// k_kp_columns_f32 decodes them into the FP64 column store:
//     kpc[e][k][r] = (double)src[e][k][r]                  an exact widening (FP32 subnormals included; NaN stays NaN, +-inf stays)
//                    + 1.0 at the unit row                 kind 0: r == d, kind 1: r == d + dof, d the DoF of entry e; ONE IEEE addition
// and nothing else: every other element is the widened float, bit for bit (no + 0.0, which would turn -0 into +0).  What the store
// then holds is what kpilqr_upload_kp_columns would have copied into it from the decoded doubles; nothing downstream can tell.
//
// A pure stream (4 bytes in, 8 out per element; no LDS, no atomics).  The DoF of an entry is its list's (list = b*dof + d of the
// device CSR kp_offsets the context already holds), so a block row is a LIST: its entries are one contiguous range of the store, and
// of the staging buffer.  The unit of work is a PAIR of consecutive elements: one 8-byte load and one 16-byte store.  An entry is 3n
// elements with n even, so a list starts on a pair in both buffers behind their hipMalloc bases and has no tail; 3n is a multiple of
// four only when dof is even (Panda: 42), so nothing wider is used -- the 16-byte store, the side with twice the bytes, is already
// the widest there is, and a 16-byte load would need a head / tail story per list.  Lanes take consecutive pairs.
//
// Compiled with -ffp-contract=off like the other streaming kernels, and with the FP32 denormal mode pinned (the Makefile): a
// subnormal float must widen to its value, not to zero.
#include "common.h"

namespace kpilqr {

#define KPC32_THREADS 256
#define KPC32_ITERS 8                                 // pairs a lane decodes per slice: a block's slice is 16 KB in, 32 KB out

// Block (x, y): slices x, x + gridDim.x, ... of lists l0 + y, l0 + y + gridDim.y, ... of the lists [l0, l1) (the whole batch: 0,
// batch*dof; a chunk of a streamed iteration: its trajectories' lists).  ppe = 3n/2 pairs per entry.  upl_first == nullptr: the staging buffer holds every entry, in store order.  Else (the partial call) upl_first [batch] is the
// third row of Ctx::kp_move as kpilqr_update_keypoints left it: the first entry of trajectory b INSIDE the compact staging buffer,
// or -1 for a trajectory that is not listed, whose lists are left alone.  Every offset is uniform over the block.
__global__ void __launch_bounds__(KPC32_THREADS)
k_kp_columns_f32(int l0, int l1, int dof, int ppe, const int *__restrict__ kp_offsets, const int *__restrict__ upl_first,
                 const float2 *__restrict__ src, double2 *__restrict__ kpc)
{
    constexpr int slice = KPC32_THREADS * KPC32_ITERS;
    for (int l = l0 + (int)blockIdx.y; l < l1; l += gridDim.y) {
        const int b = l / dof, d = l - b * dof;
        const int e0 = kp_offsets[l];
        long long s0 = e0;                                          // first entry of the list inside the staging buffer
        if (upl_first) {
            const int f = upl_first[b];
            if (f < 0) continue;
            s0 = (long long)f + (e0 - kp_offsets[b * dof]);
        }
        const long long pairs = (long long)(kp_offsets[l + 1] - e0) * ppe;
        const float2 *s = src + s0 * ppe;
        double2 *q = kpc + (long long)e0 * ppe;
        // the two unit elements of an entry: d (kind 0, row d) and n + dof + d (kind 1, row d + dof)
        const int u0 = d, u1 = 3 * dof + d;                         // (n = 2 dof)
        for (long long at = (long long)blockIdx.x * slice; at < pairs; at += (long long)gridDim.x * slice) {
            const int len = (int)(at + slice < pairs ? slice : pairs - at);
            const int ph = (int)(at % ppe);                         // the slice's first pair inside its entry (uniform: one 64-bit division per slice)
            const float2 *ss = s + at;
            double2 *qs = q + at;
#pragma unroll KPC32_ITERS
            for (int p = threadIdx.x; p < len; p += KPC32_THREADS) {
                const float2 v = ss[p];
                const int j = 2 * ((ph + p) % ppe);                 // first element of the pair inside its entry
                double2 w = make_double2((double)v.x, (double)v.y);
                if (j == u0 || j == u1) w.x = w.x + 1.0;
                if (j + 1 == u0 || j + 1 == u1) w.y = w.y + 1.0;
                qs[p] = w;
            }
        }
    }
}

// The lists [l0, l1) of the device CSR on stream s; src and upl_first as the kernel reads them.  (l1 - l0 > 0, ppe > 0)
static hipError_t launch_lists(Ctx *c, hipStream_t s, int l0, int l1, const float *src, const int *upl_first_dev)
{
    const int ppe = 3 * c->n / 2, nlists = l1 - l0;
    constexpr long long slice = (long long)KPC32_THREADS * KPC32_ITERS;
    // a canonical list has at most T entries; its slices are walked by up to 16 blocks (Panda, T = 3000, key-points every 5 steps: 7 slices)
    const long long want = ((long long)c->d.T * ppe + slice - 1) / slice;
    const dim3 grid((unsigned)(want > 16 ? 16 : want), (unsigned)(nlists < 65535 ? nlists : 65535));
    hipLaunchKernelGGL(k_kp_columns_f32, grid, dim3(KPC32_THREADS), 0, s, l0, l1, c->d.dof, ppe, (const int *)c->kp_offsets,
                       upl_first_dev, (const float2 *)src, (double2 *)(double *)c->kpc);
    return hipGetLastError();
}

// src (device): the encoded floats -- of every entry (upl_first_dev == nullptr), or of the listed trajectories' entries back to back
// (upl_first_dev [batch]: their first entries inside src, -1 for everybody else) -> the column store, at the lists' own ranges
hipError_t launch_kp_columns_f32(Ctx *c, const float *src, const int *upl_first_dev)
{
    const long long nlists = (long long)c->d.batch * c->d.dof;
    const int ppe = 3 * c->n / 2;
    if (nlists <= 0 || ppe == 0) return hipSuccess;
    if (nlists > INT32_MAX) return hipErrorInvalidValue;
    return launch_lists(c, c->stream, 0, (int)nlists, src, upl_first_dev);
}

// A chunk of a streamed iteration (kpilqr_iterate_streamed3): the lists [l0, l1) = [b0*dof, b1*dof) of the chunk's trajectories, decoded
// from `staging` -- the CONTEXT's staging buffer, in store order: the chunk's floats sit at its first entry * 3n, where its one
// upload put them -- into the same entries of the column store, on the chunk's stream s.  c is the context, never a view: its
// tables and pointers are the absolute ones.
// upl_first_dev != nullptr (kpilqr_iterate_streamed4 with upload_traj): the staging buffer holds the entries of the chunk's LISTED
// trajectories alone, back to back from the chunk's first entry on; upl_first_dev [batch] is the first entry of trajectory b inside
// the staging buffer, -1 for a trajectory that is not listed, whose lists are left alone -- the table of the partial explicit call.
hipError_t launch_kp_columns_f32_range(Ctx *c, hipStream_t s, int l0, int l1, const float *staging, const int *upl_first_dev)
{
    const long long nlists = (long long)c->d.batch * c->d.dof;
    if (l0 < 0 || l1 < l0 || l1 > nlists) return hipErrorInvalidValue;
    if (l1 == l0 || c->n == 0) return hipSuccess;
    return launch_lists(c, s, l0, l1, staging, upl_first_dev);
}

}  // namespace kpilqr
