// linearise.hip -- a2 + a4 in one pass: the key-point payload differenced and interpolated straight into the step records.
//   fd_difference  (a2)  Differentiator::DynamicsDerivatives tail, src/Differentiator/Differentiator.cpp:166-222,441-457
//   interpolate    (a4)  KeypointGenerator::InterpolateDerivatives, src/KeyPointGenerator/KeyPointGenerator.cpp:840-954
// A materialising context reached its [A|B] sequence in three streaming passes (elementwise.hip): k_fd_kp_difference (payload ->
// column store kpc), k_kpc_to_records (kpc -> the key-point steps of the records), k_interpolate (key-point columns read back out
// of the records, every step in between written).  k_fd_kp_interpolate writes every step record ONCE and reads the payload only:
// kpc is neither written nor read, and the key-point steps are not written and read back.
//
// The result is bit for bit what the three passes leave in the records, so this file is compiled with -ffp-contract=off like
// elementwise.hip: every expression is written in the reference's operation order and must not be fused (the reference's own
// test pins the interpolation bitwise, src/tests/Keypoints_Test.cpp:273-289).
#include "common.h"

namespace kpilqr {

// Decomposition of k_interpolate: a block owns LIN_TT consecutive steps of one trajectory, a thread two consecutive rows of one
// [A|B] column (n is even, records are 16-byte aligned: 16-byte stores), and walks the tile with its segment's start value and
// slope in registers.  What differs is where the endpoints of a segment come from:
//   COLS = false   the key-point ordered payload (kpilqr_upload_fd_kp): the two owned elements are 32 contiguous bytes of an
//                  entry's record, (x+, x-) pairs, plus the record's mode word; differenced here -- the `column` lambda of
//                  k_fd_kp_difference: bit `kind` of mode says one-sided (/ eps), else central (/ (2 eps)), an IEEE division
//   COLS = true    the payload IS the columns (kpilqr_upload_kp_columns): 16 bytes of kpc, no arithmetic
// segent gives the CSR entry p of the key-point at or before t (k_build_segmap); the segment's endpoints are entries p and p + 1,
// their times segmap's (s, e).  A step that is a key-point of the column's DoF gets the differenced value itself.  A thread keeps
// the last two endpoints it fetched, so inside a tile every entry is fetched once: the end of one segment is the key-point step
// that follows and the start of the next segment.
// Steps outside a DoF list's first / last key-point (segent < 0), B columns of actuators beyond the DoFs and the cost blocks of
// the record are not touched -- as in the three passes.
#define LIN_TT 16
template <bool COLS>
__global__ void __launch_bounds__(256)
k_fd_kp_interpolate(RecLayout L, int dof, int T, const int2 *__restrict__ segmap, const int *__restrict__ segent,
                    const double2 *__restrict__ src, double eps, double *__restrict__ rec, const int *__restrict__ traj)
{
    extern __shared__ __attribute__((aligned(16))) int2 ssm[];      // [dof][LIN_TT] (s, e), then int [dof][LIN_TT] entry
    const int n = L.n, m = L.m;
    const int ne = n * n + n * m;               // even: n = 2*dof
    const int b = traj ? traj[blockIdx.y] : blockIdx.y;      // a subset (kpilqr_fd_interpolate_partial): block-uniform, a scalar load
    const int t0 = blockIdx.x * LIN_TT;
    const int nt = min(LIN_TT, T - t0);
    int *sen = (int *)(ssm + dof * LIN_TT);
    double *R = rec + (size_t)b * T * L.stride;
    const int2 *sm = segmap + (size_t)b * dof * T;
    const int *se = segent + (size_t)b * dof * T;
    for (int w = threadIdx.x; w < dof * LIN_TT; w += blockDim.x) {
        const int i = w / LIN_TT, tt = w - i * LIN_TT;
        ssm[w] = (tt < nt) ? sm[(size_t)i * T + t0 + tt] : make_int2(-1, -1);
        sen[w] = (tt < nt) ? se[(size_t)i * T + t0 + tt] : -1;
    }
    __syncthreads();
    const int s2 = 3 * n + 1;                   // payload record stride in double2: 3n (x+, x-) pairs | mode, pad
    for (int e = 2 * threadIdx.x; e < ne; e += 2 * blockDim.x) {
        const int col = e / n, row = e - col * n;                // 0..n-1: A column; n..n+m-1: B column col-n
        const int kind = col < dof ? 0 : col < n ? 1 : 2;        // position | velocity | control column of DoF i
        const int i = kind == 0 ? col : kind == 1 ? col - dof : (col - n < dof ? col - n : -1);
        if (i < 0) continue;                                     // B column of an actuator beyond the DoFs: not interpolated
        const int el = kind * n + row;                           // element of an entry's 3n differenced values
        auto fetch = [&](int q) -> double2 {                     // elements el, el + 1 of CSR entry q
            if constexpr (COLS) {
                return src[((size_t)q * 3 * n + el) >> 1];
            } else {
                const double2 *r = src + (size_t)q * s2;
                const int mode = ((const int *)(r + 3 * n))[0];
                const double den = ((mode >> kind) & 1) ? eps : 2 * eps;
                const double2 a = r[el], c = r[el + 1];          // (x+, x-) of elements el and el + 1
                return make_double2((a.x - a.y) / den, (c.x - c.y) / den);
            }
        };
        int ps = -1, pe = -1;                                    // entries whose values vs, ve hold
        bool seg = false;                                        // add is the slope of segment (ps, pe)
        double2 vs = make_double2(0.0, 0.0), ve = vs, add = vs;
        for (int tt = 0; tt < nt; tt++) {
            const int p = sen[i * LIN_TT + tt];
            if (p < 0) continue;                                 // outside the DoF's first / last key-point: left alone
            const int2 sg = ssm[i * LIN_TT + tt];
            double2 v;
            if (sg.x < 0) {                                      // a key-point of this DoF: the differenced column
                v = (p == ps) ? vs : (p == pe) ? ve : fetch(p);
                if (p != ps) { ps = p; vs = v; seg = false; }
            } else {
                if (p != ps || !seg) {
                    if (p != ps) { vs = (p == pe) ? ve : fetch(p); ps = p; }
                    ve = fetch(p + 1); pe = p + 1;
                    add.x = (ve.x - vs.x) / (double)(sg.y - sg.x);
                    add.y = (ve.y - vs.y) / (double)(sg.y - sg.x);
                    seg = true;
                }
                const int t = t0 + tt;
                v.x = vs.x + ((double)(t - sg.x) * add.x);
                v.y = vs.y + ((double)(t - sg.x) * add.y);
            }
            *reinterpret_cast<double2 *>(R + (size_t)(t0 + tt) * L.stride + e) = v;     // record stride and e are even: 16-B aligned
        }
    }
}

// Works on a view of a trajectory range (kpilqr_iterate_streamed): rec, segmap and segent are the view's (shifted), batch its
// trajectories; segent holds ABSOLUTE CSR entries, so the payload / column store is addressed through its unshifted base and
// the entries a chunk touches are its own: [fdk_first, fdk_first + fdk_entries).
// traj (device, count trajectories): the listed trajectories alone, one block row each; null: the whole batch.
hipError_t launch_fd_kp_interpolate(Ctx *c, const int *traj, int count)
{
    if (c->d.batch <= 0 || c->d.T <= 0 || (traj && count <= 0)) return hipSuccess;
    dim3 grid((c->d.T + LIN_TT - 1) / LIN_TT, traj ? count : c->d.batch);
    const int ne = c->n * c->n + c->n * c->d.m;
    int threads = ((ne / 2 + 63) / 64) * 64;
    if (threads > 256) threads = 256;
    const size_t lds = (sizeof(int2) + sizeof(int)) * c->d.dof * LIN_TT;
    if (c->fd_payload == FdPayload::kp_columns)
        hipLaunchKernelGGL(k_fd_kp_interpolate<true>, grid, dim3(threads), lds, c->stream, c->L, c->d.dof, c->d.T, c->segmap, c->segent,
                           (const double2 *)c->kpc.p, c->eps, c->rec, traj);
    else
        hipLaunchKernelGGL(k_fd_kp_interpolate<false>, grid, dim3(threads), lds, c->stream, c->L, c->d.dof, c->d.T, c->segmap, c->segent,
                           (const double2 *)c->fdk_dev.p, c->eps, c->rec, traj);
    return hipGetLastError();
}

}  // namespace kpilqr
