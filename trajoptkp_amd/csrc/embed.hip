// embed.hip -- KPILQR_FLAG_EMBED_SHAPE: the device side of zero-embedding a one-tile shape (dof, m) that has no sweep kernels of its
// own into a compiled shape (dof', m') that contains it, its "carrier" (kp_t1_carrier, mfma_common.h).
//
// The context runs the carrier's sweeps unchanged; these kernels stand at the ABI boundary and only MOVE and ZERO data:
//     state row / r_x column i of the caller  ->  i            (i <  dof: positions)
//                                                 i + shift    (i >= dof: velocities; shift = dof' - dof)
//     control j                                ->  j            (a prefix)
// Padded states get zero A columns and rows, zero B rows and zero r_x columns, padded controls zero B columns: the padded block of V
// stays exactly 0, the padded block of Q_uu + lambda I is lambda I, the padded rows of K and k are exactly 0, and the real block sees
// only additions of exact zeros.  No arithmetic happens here beyond the float cast of k_extract_gains, which is
// the cast of k_gains_f32 (gains.hip): round-to-nearest-even, FP32 subnormals produced (the Makefile pins the FP32 denormal mode).
//
// Pure streams (no LDS, no atomics).  The unit of work is ONE ELEMENT -- 8 bytes for columns, rows and gains, the 16-byte (x+, x-)
// pair for the key-point ordered payload: with an odd dof the row shift is odd, so a row of doubles that is 16-byte aligned on one
// side is not on the other, and nothing wider than the element is assumed.  Lanes take consecutive DESTINATION elements of the
// payload kernels and of k_extract_gains (their stores coalesce; a lane's load is its store's mapped twin) and consecutive SOURCE
// elements of k_embed_rows (which writes the real columns alone).  Work is cut into slices whose first element is decomposed once,
// uniformly over the block, in 64 bits; the lanes then divide 32-bit offsets inside the slice.
#include "common.h"

namespace kpilqr {

#define KPE_THREADS 256
#define KPE_ITERS 8                                   // elements a lane moves per slice

__device__ __forceinline__ double kpe_zero(double) { return 0.0; }
__device__ __forceinline__ double2 kpe_zero(double2) { return make_double2(0.0, 0.0); }
// the tail unit of a key-point ordered record: int32 mode | int32 pad[3] -- the mode word is kept, the padding cleared
__device__ __forceinline__ double2 kpe_mode(double2 t)
{
    return make_double2(__longlong_as_double(__double_as_longlong(t.x) & 0xffffffffll), 0.0);
}
__device__ __forceinline__ double kpe_mode(double t) { return t; }      // (the column payload has no tail)

// The by-entry payloads.  E = double2, TAIL: records of kpilqr_fd_kp_layout, 3n (x+, x-) pairs and the mode unit; E = double: columns
// [3][n].  Block (x, y): slices x, x + gridDim.x, ... of the carrier lists y, y + gridDim.y, ... (list l = b * cdof + d of the
// carrier CSR dst_off).  A list d < dof holds the caller's list (b, d) -- the same number of entries, kpilqr_set_keypoints expanded
// the CSR so -- and reads its records from the caller's CSR src_off; a padded list (copies of the trajectory's list 0) is all zero,
// mode 0: a zero quotient 0 / (2 eps) is +0.  Of a real entry the padded rows are +0, and so is the whole control kind (kind 2) of a
// DoF d >= m: the caller's slot there is ignored by contract and may hold anything, the carrier reads it while d < m'.
template <class E, bool TAIL>
__global__ void __launch_bounds__(KPE_THREADS)
k_embed_entries(int nlists, int cdof, int dof, int m, const int *__restrict__ src_off, const int *__restrict__ dst_off,
                const E *__restrict__ src, E *__restrict__ dst)
{
    constexpr int slice = KPE_THREADS * KPE_ITERS;
    const int cn = 2 * cdof, n = 2 * dof, shift = cdof - dof;
    const int ud = 3 * cn + (TAIL ? 1 : 0), us = 3 * n + (TAIL ? 1 : 0);      // units per carrier / caller entry
    for (int l = blockIdx.y; l < nlists; l += gridDim.y) {
        const int b = l / cdof, d = l - b * cdof;
        const int e0 = dst_off[l];
        const long long units = (long long)(dst_off[l + 1] - e0) * ud;
        const bool real = d < dof;
        const E *s = src + (real ? (long long)src_off[b * dof + d] * us : 0);
        E *q = dst + (long long)e0 * ud;
        const bool ctrl = d < m;
        for (long long at = (long long)blockIdx.x * slice; at < units; at += (long long)gridDim.x * slice) {
            const int len = (int)(at + slice < units ? slice : units - at);
            const long long j0 = at / ud;                       // the slice's first entry inside the list, and unit inside that entry
            const int w0 = (int)(at - j0 * ud);
#pragma unroll KPE_ITERS
            for (int p = threadIdx.x; p < len; p += KPE_THREADS) {
                int w = w0 + p;
                const int dj = w / ud;
                w -= dj * ud;
                const E *se = s + (j0 + dj) * us;
                E v = kpe_zero(E{});
                if (real) {
                    if (TAIL && w == 3 * cn) v = kpe_mode(se[3 * n]);
                    else {
                        const int kind = w / cn, row = w - kind * cn;
                        const int sr = row < dof ? row : (row >= cdof && row < cdof + dof) ? row - shift : -1;
                        if (sr >= 0 && (kind < 2 || ctrl)) v = se[kind * n + sr];
                    }
                }
                q[at + p] = v;
            }
        }
    }
}

template <class E, bool TAIL>
static hipError_t launch_entries(Ctx *c, const void *src, void *dst)
{
    const long long nlists = (long long)c->d.batch * c->d.dof;
    if (nlists <= 0) return hipSuccess;
    if (nlists > INT32_MAX) return hipErrorInvalidValue;
    constexpr long long slice = (long long)KPE_THREADS * KPE_ITERS;
    // a canonical list has at most T entries; its slices are walked by up to 16 blocks
    const long long want = ((long long)c->d.T * (3 * c->n + 1) + slice - 1) / slice;
    const dim3 grid((unsigned)(want > 16 ? 16 : want), (unsigned)(nlists < 65535 ? nlists : 65535));
    hipLaunchKernelGGL((k_embed_entries<E, TAIL>), grid, dim3(KPE_THREADS), 0, c->stream, (int)nlists, c->d.dof, c->embed.dof, c->embed.m,
                       (const int *)c->emb_offsets, (const int *)c->kp_offsets, (const E *)src, (E *)dst);
    return hipGetLastError();
}

hipError_t launch_embed_fd_kp(Ctx *c, const void *src) { return launch_entries<double2, true>(c, src, (char *)c->fdk_dev); }
hipError_t launch_embed_kp_columns(Ctx *c, const double *src) { return launch_entries<double, false>(c, src, (double *)c->kpc); }

// Rows of a matrix sequence (r_x: rows of n state columns; r_u, u_nom: rows of m controls): element (row, j) of src [rows][cols] goes
// to column j (j < split) or j + shift (j >= split) of row `row` of dst [rows][dst_cols].  Only those elements are written: the
// padding of dst was zeroed with the buffer and stays +0.  total = rows * cols.
__global__ void __launch_bounds__(KPE_THREADS)
k_embed_rows(long long total, int cols, int dst_cols, int split, int shift, const double *__restrict__ src, double *__restrict__ dst)
{
    constexpr int slice = KPE_THREADS * KPE_ITERS;
    for (long long at = (long long)blockIdx.x * slice; at < total; at += (long long)gridDim.x * slice) {
        const int len = (int)(at + slice < total ? slice : total - at);
        const long long row0 = at / cols;
        const int j0 = (int)(at - row0 * cols);
#pragma unroll KPE_ITERS
        for (int p = threadIdx.x; p < len; p += KPE_THREADS) {
            int j = j0 + p;
            const int dr = j / cols;
            j -= dr * cols;
            dst[(row0 + dr) * dst_cols + (j < split ? j : j + shift)] = src[at + p];
        }
    }
}

hipError_t launch_embed_rows(Ctx *c, long long rows, int cols, int dst_cols, int split, int shift, const double *src, double *dst)
{
    const long long total = rows * cols;
    if (total <= 0) return hipSuccess;
    if (cols + shift > dst_cols || split > cols || shift < 0) return hipErrorInvalidValue;
    constexpr long long slice = (long long)KPE_THREADS * KPE_ITERS;
    const long long want = (total + slice - 1) / slice;
    hipLaunchKernelGGL(k_embed_rows, dim3((unsigned)(want > 4096 ? 4096 : want)), dim3(KPE_THREADS), 0, c->stream, total, cols, dst_cols,
                       split, shift, src, dst);
    return hipGetLastError();
}

__device__ __forceinline__ void kpe_store(double *d, double v) { *d = v; }
__device__ __forceinline__ void kpe_store(float *d, double v) { *d = (float)v; }      // the cast of k_gains_f32

// The outputs back in the caller's shape: dst [R][n][m] compact (R = count * rows matrices: K of every step, or with n = 1 the rows
// of k and U_alpha) gathered from src [R][src_n][src_m]; matrix row i is read at i (i < split) or i + shift.  total = R * n * m.
template <class D>
__global__ void __launch_bounds__(KPE_THREADS)
k_extract_gains(long long total, int n, int m, int src_n, int src_m, int split, int shift, const double *__restrict__ src, D *__restrict__ dst)
{
    constexpr int slice = KPE_THREADS * KPE_ITERS;
    for (long long at = (long long)blockIdx.x * slice; at < total; at += (long long)gridDim.x * slice) {
        const int len = (int)(at + slice < total ? slice : total - at);
        const long long q0 = at / m;                      // (matrix, row) pair of the slice's first element ...
        const int j0 = (int)(at - q0 * m);
        const long long R0 = q0 / n;                      // ... its matrix and its row inside it
        const int i0 = (int)(q0 - R0 * n);
#pragma unroll KPE_ITERS
        for (int p = threadIdx.x; p < len; p += KPE_THREADS) {
            int j = j0 + p;
            const int dq = j / m;
            j -= dq * m;
            int i = i0 + dq;
            const int dR = i / n;
            i -= dR * n;
            kpe_store(dst + at + p, src[((R0 + dR) * src_n + (i < split ? i : i + shift)) * src_m + j]);
        }
    }
}

hipError_t launch_extract_gains(Ctx *c, int count, long long rows, int n, int m, int src_n, int src_m, int split, int shift,
                                const double *src, void *dst, bool as_f32)
{
    const long long total = (long long)count * rows * n * m;
    if (total <= 0) return hipSuccess;
    if (n + shift > src_n || m > src_m || split > n || shift < 0) return hipErrorInvalidValue;
    constexpr long long slice = (long long)KPE_THREADS * KPE_ITERS;
    const long long want = (total + slice - 1) / slice;
    const dim3 grid((unsigned)(want > 4096 ? 4096 : want)), block(KPE_THREADS);
    if (as_f32) hipLaunchKernelGGL((k_extract_gains<float>), grid, block, 0, c->stream, total, n, m, src_n, src_m, split, shift, src, (float *)dst);
    else hipLaunchKernelGGL((k_extract_gains<double>), grid, block, 0, c->stream, total, n, m, src_n, src_m, split, shift, src, (double *)dst);
    return hipGetLastError();
}

}  // namespace kpilqr
