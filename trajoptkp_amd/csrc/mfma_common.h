// mfma_common.h -- device helpers shared by the FP64 MFMA kernels (riccati_mfma.hip, forward_mfma.hip,
// tiled_mfma.hip, tiled_wide.hip, fused_mfma.hip): the primitive layer (tile type, matrix instruction, bounds-checked
// buffer accesses, LDS tile images, record tile sources, the one-tile LDS map), a ~1 ulp reciprocal, the running
// inverse, and the slow path of the backward pass (Eigen's pivoted LDLT + explicit inverse).
#pragma once
#include "common.h"

namespace kpilqr {

// ---- the primitive layer: the one copy of what every sweep unit is written in ---------------------------------------------
typedef double d4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// D = A*B + C on the FP64 matrix core, 16x16 output, 4 rows of the contraction per instruction.
#define KP_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
// byte offset that lies outside every buffer descriptor used here: the load returns 0, the store is dropped
#define KP_OOB 0x7ffffff0
// LDS tile image: 256 doubles, register r of lane l at [r*64 + l]; 16 x 17 padded row-major tile (transposed reads without bank conflicts)
#define KP_TILE 256
#define KP_TPAD 272

// Bounds-checked buffer accesses: a lane whose tile element is a structural zero carries an out-of-range offset and gets 0
// from the hardware (no select on the loaded value, so nothing consumes it until the product that needs it).
__device__ __forceinline__ double kp_bld(__amdgpu_buffer_rsrc_t r, int byte_off)
{
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, 0));
}
// the same with a wave-uniform byte offset in the instruction's scalar operand: ONE descriptor per array and trajectory,
// the step selected by an SGPR, instead of a descriptor rebuilt (64-bit address arithmetic, ~8 SALU) per array and step
__device__ __forceinline__ double kp_blds(__amdgpu_buffer_rsrc_t r, int byte_off, int soff)
{
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, soff, 0));
}
// two consecutive doubles with one request (16-byte aligned)
__device__ __forceinline__ void kp_bld2s(__amdgpu_buffer_rsrc_t r, int byte_off, int soff, double &a, double &b)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, soff, 0);
    const u32x2 lo = {v.x, v.y}, hi = {v.z, v.w};
    a = __builtin_bit_cast(double, lo); b = __builtin_bit_cast(double, hi);
}
__device__ __forceinline__ void kp_bld2(__amdgpu_buffer_rsrc_t r, int byte_off, double &a, double &b) { kp_bld2s(r, byte_off, 0, a, b); }
__device__ __forceinline__ void kp_bst(double x, __amdgpu_buffer_rsrc_t r, int byte_off)
{
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, x), r, byte_off, 0, 0);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t kp_rsrc(const void *p, int bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, bytes, 0x00020000);
}

// acc + Y'X over NC 4-row chunks: the one primitive of these kernels (tiles in the accumulator layout are their own
// transpose as the A operand and the next B operand as they are).
template <int NC>
__device__ __forceinline__ d4 kp_P(const d4 &Y, const d4 &X, d4 acc)
{
    acc = KP_MFMA(Y.x, X.x, acc);
    if (NC > 1) acc = KP_MFMA(Y.y, X.y, acc);
    if (NC > 2) acc = KP_MFMA(Y.z, X.z, acc);
    if (NC > 3) acc = KP_MFMA(Y.w, X.w, acc);
    return acc;
}
// the same over `nc` chunks known at run time (nc is wave-uniform)
__device__ __forceinline__ d4 kp_Pn(const d4 &Y, const d4 &X, d4 acc, int nc)
{
    acc = KP_MFMA(Y.x, X.x, acc);
    if (nc > 1) acc = KP_MFMA(Y.y, X.y, acc);
    if (nc > 2) acc = KP_MFMA(Y.z, X.z, acc);
    if (nc > 3) acc = KP_MFMA(Y.w, X.w, acc);
    return acc;
}

// A tile between registers and its LDS image; <NC>: the first NC registers only (the others read as 0)
__device__ __forceinline__ d4 kp_lds_tile(const double *t, int lane)
{
    d4 v; v.x = t[lane]; v.y = t[64 + lane]; v.z = t[128 + lane]; v.w = t[192 + lane];
    return v;
}
__device__ __forceinline__ void kp_lds_store(double *t, int lane, const d4 &v)
{
    t[lane] = v.x; t[64 + lane] = v.y; t[128 + lane] = v.z; t[192 + lane] = v.w;
}
template <int NC> __device__ __forceinline__ d4 kp_lds_tile(const double *t, int lane)
{
    d4 v = {0.0, 0.0, 0.0, 0.0};
    v.x = t[lane];
    if constexpr (NC > 1) v.y = t[64 + lane];
    if constexpr (NC > 2) v.z = t[128 + lane];
    if constexpr (NC > 3) v.w = t[192 + lane];
    return v;
}
template <int NC> __device__ __forceinline__ void kp_lds_store(double *t, int lane, const d4 &v)
{
    t[lane] = v.x;
    if constexpr (NC > 1) t[64 + lane] = v.y;
    if constexpr (NC > 2) t[128 + lane] = v.z;
    if constexpr (NC > 3) t[192 + lane] = v.w;
}

// register R of a tile, R at compile time / r at run time
template <int R> __device__ __forceinline__ void kp_set_reg(d4 &v, double x) { if (R == 0) v.x = x; else if (R == 1) v.y = x; else if (R == 2) v.z = x; else v.w = x; }
__device__ __forceinline__ void kp_set_reg(d4 &v, int r, double x)
{
    if (r == 0) v.x = x; else if (r == 1) v.y = x; else if (r == 2) v.z = x; else v.w = x;
}

// LDS map (doubles) of the one-tile backward sweeps.  KP_MS: row stride of the Quu image; KP_MZ: column stride of the Quz image
// (odd -> conflict-free column reads); KP_VS: row stride of the transpose image; behind KP_LDS_SLOW the work area of the slow path.
#define KP_MS 16
#define KP_MZ 17
#define KP_VS 17
#define KP_LDS_Q 0
#define KP_LDS_Z (KP_LDS_Q + 16 * KP_MS)
#define KP_LDS_V (KP_LDS_Z + 16 * KP_MZ)
#define KP_LDS_SLOW (KP_LDS_V + 16 * KP_VS)

// Tiles of a step record for the tiled sweeps (bounds-checked: structural zeros come back as 0).  Register r of a tile in the
// accumulator layout: element (16 ti + 4 r + q, 16 tj + c); the *1 loaders fetch one register, so that a sweep can spread its
// requests under its products.  A control index spans the control tiles tj = 0, 1 (tiled_mfma.hip, m <= 8: tile 0 only).
struct KpTileSrc { int n, m; int off_A, off_B, off_lxx, off_lx, off_luu, off_lu; };

__device__ __forceinline__ double kp_ld_Lzz1(__amdgpu_buffer_rsrc_t rs, const KpTileSrc &S, int ti, int tj, int r, int q, int c)
{
    const int row = 16 * ti + 4 * r + q, col = 16 * tj + c, n = S.n;
    const int off = (row < n && col < n) ? 8 * (S.off_lxx + row * n + col)
                  : (col == n && row < n) ? 8 * (S.off_lx + row)
                  : (row == n && col < n) ? 8 * (S.off_lx + col) : KP_OOB;
    return kp_bld(rs, off);
}
__device__ __forceinline__ double kp_ld_Fz1(__amdgpu_buffer_rsrc_t rs, const KpTileSrc &S, int ti, int tj, int r, int q, int c)
{
    const int row = 16 * ti + 4 * r + q, col = 16 * tj + c, n = S.n;
    return kp_bld(rs, (row < n && col < n) ? 8 * (S.off_A + col * n + row) : KP_OOB);
}
// B(row tile ti, control tile tj)
__device__ __forceinline__ double kp_ld_Fu1(__amdgpu_buffer_rsrc_t rs, const KpTileSrc &S, int ti, int tj, int r, int q, int c)
{
    const int row = 16 * ti + 4 * r + q, col = 16 * tj + c;
    return kp_bld(rs, (row < S.n && col < S.m) ? 8 * (S.off_B + col * S.n + row) : KP_OOB);
}
// Luz(control tile tj, state tile tw): l_u in column n
__device__ __forceinline__ double kp_ld_Luz1(__amdgpu_buffer_rsrc_t rs, const KpTileSrc &S, int tj, int tw, int r, int q, int c)
{
    const int row = 16 * tj + 4 * r + q, col = 16 * tw + c;
    return kp_bld(rs, (row < S.m && col == S.n) ? 8 * (S.off_lu + row) : KP_OOB);
}
__device__ __forceinline__ double kp_ld_Luu1(__amdgpu_buffer_rsrc_t rs, const KpTileSrc &S, int ta, int tb, int r, int q, int c)
{
    const int row = 16 * ta + 4 * r + q, col = 16 * tb + c;
    return kp_bld(rs, (row < S.m && col < S.m) ? 8 * (S.off_luu + row * S.m + col) : KP_OOB);
}
#define KP_X(NAME) \
__device__ __forceinline__ d4 kp_ld_##NAME(__amdgpu_buffer_rsrc_t rs, const KpTileSrc &S, int ti, int tj, int q, int c) \
{ \
    d4 o = {kp_ld_##NAME##1(rs, S, ti, tj, 0, q, c), kp_ld_##NAME##1(rs, S, ti, tj, 1, q, c), kp_ld_##NAME##1(rs, S, ti, tj, 2, q, c), kp_ld_##NAME##1(rs, S, ti, tj, 3, q, c)}; \
    return o; \
}
KP_X(Lzz) KP_X(Fz) KP_X(Fu) KP_X(Luz) KP_X(Luu)
#undef KP_X

// 1/x to ~1 ulp: v_rcp_f64 seed + two Newton steps (the pivots are O(lambda)..O(1): no scaling needed; a
// non-positive or non-finite pivot is caught by the callers' `pos` test and takes the slow path).
__device__ __forceinline__ double kp_rcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    return r;
}

// One-tile shapes (n + 1 <= 16) that have their own backward / fused kernel instantiations: Panda reaching and push_soft
// (14,7), Acrobot and piston (4,1), hopper and floating cube (12,3), pentabot (10,3) -- the joint / actuator counts of the
// reference's TaskConfigs.  Everything else goes to the tiled kernels (any n + 2 <= 64, num_ctrl <= 8).
#define KP_T1_SHAPES(X) X(14, 7) X(4, 1) X(12, 3) X(10, 3)
static inline bool kp_t1_shape(int n, int m)
{
#define KP_X(NN, MM) if (n == NN && m == MM) return true;
    KP_T1_SHAPES(KP_X)
#undef KP_X
    return false;
}
// KPILQR_FLAG_EMBED_SHAPE: the carrier of a caller's (dof, m) -- the compiled shape with the smallest n', then the smallest m', that
// contains it (dof <= dof', m <= m'); the caller's problem is zero-embedded into it at the ABI boundary (embed.hip).  A shape of the
// table is its own carrier.  false: none contains it (or m > dof, which no fused sweep takes).
static inline bool kp_t1_carrier(int dof, int m, int *carrier_dof, int *carrier_m)
{
    int bn = 0, bm = 0;
    if (dof < 1 || m < 1 || m > dof) return false;
#define KP_X(NN, MM) if (2 * dof <= NN && m <= MM && (!bn || NN < bn || (NN == bn && MM < bm))) { bn = NN; bm = MM; }
    KP_T1_SHAPES(KP_X)
#undef KP_X
    if (!bn) return false;
    *carrier_dof = bn / 2; *carrier_m = bm;
    return true;
}

// Running inverse of Q = Quu + lambda I (m x m, rows/cols < 4*NCU of a tile): Newton-Schulz steps
// Xinv <- Xinv + Xinv (I - Q Xinv) on the matrix core, 4 MFMAs each, quadratic convergence.  The number of steps is
// chosen from the measured residual so that the last one ends below 1e-15 (bound on the row sums of |I - Q Xinv|:
// m * max entry).  Returns false, leaving Xinv untouched, when the residual is too large to converge in four
// steps (the caller then factorises).  Q and Xinv are symmetric up to rounding, so Q'X = QX and X'R = XR.
//
// That count is normwise: e is the residual's largest entry.  An entry of the inverse that is small beside the diagonal and has
// itself moved by a relative d since the last step (the coupling of a weak control to a strong one, where the units of the controls
// are decades apart and drift) leaves e untouched, and every second-order step multiplies ITS relative error by twice the normwise
// error of the moment only: d 2e after one step, d 4e^3 after two, d 8e^7, d 16e^15.  The row of K = -X Quz of the weak control
// inherits it through X_j0 Quz_0.  So the first step also looks at every entry: where what the bin's steps will leave of its own
// movement is over KP_NS_MOVE_TOL of the entry, AND the movement is under KP_NS_MOVE_NEGL of (largest residual entry) x (largest
// entry of X) -- invisible to the count --, one more step follows the bin's own.  The second condition keeps entries that are small
// by cancellation, whose movement is of the size of everybody's, from buying a step on every dense matrix.
// (mirrored in tests/_refresh.py, MOVE_TOL / MOVE_NEGL; tests/test_gpu_blockwise.py is what sees it)
#define KP_NS_MOVE_TOL 1.0e-14
#define KP_NS_MOVE_NEGL 1.0e-2
__device__ __forceinline__ double kp_wave_max(double v)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double kp_ns_move_c(int iters, double e)     // 2e, 4e^3, 8e^7, 16e^15
{
    const double e2 = e * e, e3 = e2 * e, e7 = e3 * e3 * e;
    return iters == 1 ? 2.0 * e : iters == 2 ? 4.0 * e3 : iters == 3 ? 8.0 * e7 : 16.0 * e7 * e7 * e;
}
__device__ __forceinline__ bool kp_ns_moved(double x0, double x1, double c, double negl)
{
    const double d = fabs(x1 - x0);
    return d * c > KP_NS_MOVE_TOL * fabs(x1) && d < negl;
}
template <int NCU>
__device__ __forceinline__ bool kp_inverse_refresh(const d4 &Qr, const d4 &Iu, d4 &Xinv, int m)
{
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    d4 R = Iu - kp_P<NCU>(Qr, Xinv, zero);
    double rmax = fabs(R.x);
    if (NCU > 1) rmax = fmax(rmax, fabs(R.y));
    if (NCU > 2) rmax = fmax(rmax, fabs(R.z));
    if (NCU > 3) rmax = fmax(rmax, fabs(R.w));
    const double e = (double)m * rmax;
    // (thresholds and step counts mirrored in tests/_refresh.py, family "plain")
    if (__builtin_amdgcn_ballot_w64(!(e < 0.11)) != 0) return false;
    const int iters = (__builtin_amdgcn_ballot_w64(e >= 1.3e-2) != 0) ? 4
                    : (__builtin_amdgcn_ballot_w64(e >= 1.7e-4) != 0) ? 3
                    : (__builtin_amdgcn_ballot_w64(e >= 3.0e-8) != 0) ? 2 : 1;
    const d4 X0 = Xinv;
    double xmax = fabs(X0.x);
    if (NCU > 1) xmax = fmax(xmax, fabs(X0.y));
    if (NCU > 2) xmax = fmax(xmax, fabs(X0.z));
    if (NCU > 3) xmax = fmax(xmax, fabs(X0.w));
    const double ru = kp_wave_max(rmax);
    const double c = kp_ns_move_c(iters, (double)m * ru), negl = KP_NS_MOVE_NEGL * ru * kp_wave_max(xmax);
    Xinv = kp_P<NCU>(Xinv, R, Xinv);
    bool moved = kp_ns_moved(X0.x, Xinv.x, c, negl);
    if (NCU > 1) moved = moved || kp_ns_moved(X0.y, Xinv.y, c, negl);
    if (NCU > 2) moved = moved || kp_ns_moved(X0.z, Xinv.z, c, negl);
    if (NCU > 3) moved = moved || kp_ns_moved(X0.w, Xinv.w, c, negl);
    const bool extra = __builtin_amdgcn_ballot_w64(moved) != 0;
    if (iters > 1) {
        R = Iu - kp_P<NCU>(Qr, Xinv, zero); Xinv = kp_P<NCU>(Xinv, R, Xinv);
        if (iters > 2) {
            R = Iu - kp_P<NCU>(Qr, Xinv, zero); Xinv = kp_P<NCU>(Xinv, R, Xinv);
            if (iters > 3) { R = Iu - kp_P<NCU>(Qr, Xinv, zero); Xinv = kp_P<NCU>(Xinv, R, Xinv); }
        }
    }
    if (extra) { R = Iu - kp_P<NCU>(Qr, Xinv, zero); Xinv = kp_P<NCU>(Xinv, R, Xinv); }
    return true;
}

// The same with (1) a first guess extrapolated from the last two inverses, 2 Xinv - Xprev: between key-points the
// inverse moves smoothly from step to step, so the residual of the extrapolation is the SECOND difference (Panda bench
// workload: median 8e-7 against 4e-5 for the plain previous inverse; at a key-point, where the slopes of A and B change,
// it falls back to first order), and (2) a third-order step issued BEFORE the residual is looked at:
//     Y = X + X R,  X <- X + Y R   ( = X (I + R + R^2), error e^3; Y is symmetric like X: X R = X - X Q X )
// 6 MFMAs in a straight line and one branch when e < 2e-5 (e^3 < 1e-14); beyond that, second-order steps continue
// from the third-order result (residual e^3).  Shorter dependent chain than two second-order steps (3 transitions
// against 4, one residual test against four, 34.4 MFMAs per step against 36): backward sweep of one trajectory
// 3.30 -> 3.11 ms (consumer wave of the triple, where the chain is the critical path), B = 1024 one-wave 5.28 -> 5.19 ms.
template <int NCU>
__device__ __forceinline__ bool kp_inverse_refresh_p(const d4 &Qr, const d4 &Iu, d4 &Xinv, d4 &Xprev, int m)
{
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    d4 X0 = Xinv;
    X0.x = __builtin_fma(2.0, Xinv.x, -Xprev.x);
    if (NCU > 1) X0.y = __builtin_fma(2.0, Xinv.y, -Xprev.y);
    if (NCU > 2) X0.z = __builtin_fma(2.0, Xinv.z, -Xprev.z);
    if (NCU > 3) X0.w = __builtin_fma(2.0, Xinv.w, -Xprev.w);
    d4 R = Iu - kp_P<NCU>(Qr, X0, zero);
    d4 Y = kp_P<NCU>(X0, R, X0);
    Y = kp_P<NCU>(Y, R, X0);
    double rmax = fabs(R.x);
    if (NCU > 1) rmax = fmax(rmax, fabs(R.y));
    if (NCU > 2) rmax = fmax(rmax, fabs(R.z));
    if (NCU > 3) rmax = fmax(rmax, fabs(R.w));
    const double e = (double)m * rmax;
    // (thresholds and step counts mirrored in tests/_refresh.py, family "p")
    if (__builtin_amdgcn_ballot_w64(!(e < 2.0e-5)) != 0) {
        if (__builtin_amdgcn_ballot_w64(!(e < 0.11)) != 0) return false;
        const int iters = (__builtin_amdgcn_ballot_w64(e >= 1.3e-2) != 0) ? 3 : (__builtin_amdgcn_ballot_w64(e >= 1.7e-4) != 0) ? 2 : 1;
        R = Iu - kp_P<NCU>(Qr, Y, zero); Y = kp_P<NCU>(Y, R, Y);
        if (iters > 1) {
            R = Iu - kp_P<NCU>(Qr, Y, zero); Y = kp_P<NCU>(Y, R, Y);
            if (iters > 2) { R = Iu - kp_P<NCU>(Qr, Y, zero); Y = kp_P<NCU>(Y, R, Y); }
        }
    }
    Xprev = Xinv;
    Xinv = Y;
    return true;
}

// The same on the NEGATED inverse N = -(Quu + lambda I)^-1 (what the fused backward sweep carries): the residual
// R = I - Q X = I + Q N is the MFMA accumulator started at I -- no VALU between the products of the chain -- and the gains
// K = -X = N Quz come out with their sign.  Everything else as kp_inverse_refresh_p (N (I + R + R^2), extrapolated start).
// steps (optional): the number of second-order steps that followed the third-order one (0..3; -1 when it gave up).
// KINK (the step right below a key-point, known statically in the segment-loop forms: the peeled step): the slopes of A and B
// change there, the extrapolated first guess is off by a FIRST difference again (residual median ~4e-5 instead of ~8e-7) and the
// third-order step alone is not enough on most such steps (round 3: 18 % of all steps ran a second-order step behind it: 4 MFMAs,
// a residual test and a chain transition).  One more term of the series instead -- N0 (I + R + R^2 + R^3), error e^4, two more
// MFMAs in the same straight line -- is enough up to e < 1.7e-4 (e^4 < 1e-15).
#ifndef KP_SERIES4
#define KP_SERIES4 1                // 0: a second-order step wherever the third-order series does not reach 1e-15 (round 4 before the last day; A/B builds)
#endif
// SER4 (the consumer waves of the wave pairs / triple): see the fourth term below
template <int NCU, bool KINK = false, bool SER4 = false>
__device__ __forceinline__ bool kp_inverse_refresh_n(const d4 &Qr, const d4 &Iu, d4 &Ninv, d4 &Nprev, int m, int *steps = nullptr)
{
    if (steps) *steps = 0;
    d4 N0 = Ninv;
    N0.x = __builtin_fma(2.0, Ninv.x, -Nprev.x);
    if (NCU > 1) N0.y = __builtin_fma(2.0, Ninv.y, -Nprev.y);
    if (NCU > 2) N0.z = __builtin_fma(2.0, Ninv.z, -Nprev.z);
    if (NCU > 3) N0.w = __builtin_fma(2.0, Ninv.w, -Nprev.w);
    d4 R = kp_P<NCU>(Qr, N0, Iu);                     // I + Q N0
    d4 Y = kp_P<NCU>(N0, R, N0);
    Y = kp_P<NCU>(Y, R, N0);
    if constexpr (KINK) Y = kp_P<NCU>(Y, R, N0);      // N0 (I + R + R^2 + R^3)
    double rmax = fabs(R.x);
    if (NCU > 1) rmax = fmax(rmax, fabs(R.y));
    if (NCU > 2) rmax = fmax(rmax, fabs(R.z));
    if (NCU > 3) rmax = fmax(rmax, fabs(R.w));
    const double e = (double)m * rmax;
    // (thresholds, series terms and step counts mirrored in tests/_refresh.py, families "n", "n_kink", "n_ser4")
    if (__builtin_amdgcn_ballot_w64(!(e < (KINK ? 1.7e-4 : 2.0e-5))) != 0) {
        if (__builtin_amdgcn_ballot_w64(!(e < 0.11)) != 0) { if (steps) *steps = -1; return false; }
        if (!KINK && SER4 && KP_SERIES4 && __builtin_amdgcn_ballot_w64(e >= 1.7e-4) == 0) {
            // 2e-5 <= e < 1.7e-4 in a consumer wave, which does not know at compile time that it is on the step below a key-point:
            // the fourth term of the series, two products, instead of a second-order step, four -- the measured residual says it is
            // enough (e^4 < 1e-15).  2.92 against 2.96 ms at 512 trajectories.  (In the one-wave sweeps -- the general form meets
            // such steps at every DoF's key-points -- it measured -0.03 ... +0.10 ms: left as it was there.)
            if (steps) *steps = 1;
            Y = kp_P<NCU>(Y, R, N0);
        } else {
        // second-order steps behind the series: its residual is e^3 (e^4), squared by every step, to end below 1e-15
        const int iters = KINK ? ((__builtin_amdgcn_ballot_w64(e >= 1.3e-2) != 0) ? 2 : 1)
                               : (__builtin_amdgcn_ballot_w64(e >= 1.3e-2) != 0) ? 3 : (__builtin_amdgcn_ballot_w64(e >= 1.7e-4) != 0) ? 2 : 1;
        if (steps) *steps = iters;
        R = kp_P<NCU>(Qr, Y, Iu); Y = kp_P<NCU>(Y, R, Y);
        if (iters > 1) {
            R = kp_P<NCU>(Qr, Y, Iu); Y = kp_P<NCU>(Y, R, Y);
            if (iters > 2) { R = kp_P<NCU>(Qr, Y, Iu); Y = kp_P<NCU>(Y, R, Y); }
        }
        }
    }
    Nprev = Ninv;
    Ninv = Y;
    return true;
}

// kp_inverse_refresh_n for the uniform one-wave sweeps, with the state a sweep really carries: rows behind 4 NCU of the m x m inverse
// are structural zeros, so the running inverse and the one before it are their NCU live registers (Nh, Np) and the first guess is
// written into the head of N0, a tile that lives across the steps for nothing else and whose tail the caller zeroed once.  N0 is the
// accumulator input of the series products, which write elsewhere: its tail is never written.  Same products and FMAs in the same
// order as kp_inverse_refresh_n: same bits in the heads (the tails never entered a head: row i of a product is row i of its inputs).
template <int NCU, bool KINK>
__device__ __forceinline__ bool kp_inverse_refresh_heads(const d4 &Qr, const d4 &Iu, double (&Nt)[2], double (&Nh)[NCU], double (&Np)[NCU], int m, int *steps = nullptr)
{
    static_assert(NCU <= 2, "heads: one or two live registers");
    if (steps) *steps = 0;
    d4 N0;
    N0.x = __builtin_fma(2.0, Nh[0], -Np[0]);
    if constexpr (NCU > 1) N0.y = __builtin_fma(2.0, Nh[1], -Np[1]); else N0.y = Nt[0];
    N0.z = Nt[0]; N0.w = Nt[1];
    // (no instruction: the tile stays ONE value carried from step to step in the compiler's eyes.  Left to see that every step overwrites
    // the head, it keeps the tile of the set-up aside and copies all of it in front of every series.)
    d4 R = kp_P<NCU>(Qr, N0, Iu);                     // I + Q N0
    d4 Y = kp_P<NCU>(N0, R, N0);
    Y = kp_P<NCU>(Y, R, N0);
    if constexpr (KINK) Y = kp_P<NCU>(Y, R, N0);      // N0 (I + R + R^2 + R^3)
    asm volatile("" :: "v"(N0));                      // (see above: N0 outlives the series)
    double rmax = fabs(R.x);
    if constexpr (NCU > 1) rmax = fmax(rmax, fabs(R.y));
    const double e = (double)m * rmax;
    // (thresholds, series terms and step counts: kp_inverse_refresh_n's, families "n" and "n_kink" of tests/_refresh.py)
    if (__builtin_amdgcn_ballot_w64(!(e < (KINK ? 1.7e-4 : 2.0e-5))) != 0) {
        if (__builtin_amdgcn_ballot_w64(!(e < 0.11)) != 0) { if (steps) *steps = -1; return false; }
        const int iters = KINK ? ((__builtin_amdgcn_ballot_w64(e >= 1.3e-2) != 0) ? 2 : 1)
                               : (__builtin_amdgcn_ballot_w64(e >= 1.3e-2) != 0) ? 3 : (__builtin_amdgcn_ballot_w64(e >= 1.7e-4) != 0) ? 2 : 1;
        if (steps) *steps = iters;
        R = kp_P<NCU>(Qr, Y, Iu); Y = kp_P<NCU>(Y, R, Y);
        if (iters > 1) {
            R = kp_P<NCU>(Qr, Y, Iu); Y = kp_P<NCU>(Y, R, Y);
            if (iters > 2) { R = kp_P<NCU>(Qr, Y, Iu); Y = kp_P<NCU>(Y, R, Y); }
        }
    }
    Np[0] = Nh[0]; Nh[0] = Y.x;
    if constexpr (NCU > 1) { Np[1] = Nh[1]; Nh[1] = Y.y; }
    return true;
}

// Unpivoted LDL' of an m x m SPD matrix, done redundantly by every lane from a broadcast image (`qel(i,j)` returns
// element (i,j)): L (unit lower, strictly lower part stored) and the reciprocals of D.  Returns false when a pivot is
// not positive -- the callers then report the PD failure (checked steps) or take the pivoted slow path.
template <int M, class QEl>
__device__ __forceinline__ bool kp_ldl_factor(QEl qel, double (&Lm)[M][M], double (&rd)[M])
{
    double dd[M];
    bool pos = true;
#pragma unroll
    for (int j = 0; j < M; j++) {
        double w[M];
        double dj = qel(j, j);
#pragma unroll
        for (int kk = 0; kk < j; kk++) { w[kk] = Lm[j][kk] * dd[kk]; dj -= Lm[j][kk] * w[kk]; }
        dd[j] = dj;
        pos = pos && (dj > 0.0);
        const double rj = kp_rcp(dj);
        rd[j] = rj;
#pragma unroll
        for (int i = j + 1; i < M; i++) {
            double v = qel(i, j);
#pragma unroll
            for (int kk = 0; kk < j; kk++) v -= Lm[i][kk] * w[kk];
            Lm[i][j] = v * rj;
        }
    }
    return pos;
}
// x <- (L D L')^-1 x
template <int M>
__device__ __forceinline__ void kp_ldl_solve(const double (&Lm)[M][M], const double (&rd)[M], double (&x)[M])
{
#pragma unroll
    for (int j = 0; j < M; j++) {            // L y = z
#pragma unroll
        for (int i = j + 1; i < M; i++) x[i] -= Lm[i][j] * x[j];
    }
#pragma unroll
    for (int i = 0; i < M; i++) x[i] *= rd[i];   // D
#pragma unroll
    for (int j = M - 1; j >= 0; j--) {       // L' x = y
#pragma unroll
        for (int i = 0; i < j; i++) x[i] -= Lm[j][i] * x[j];
    }
}

// Eigen's LDLT (symmetric pivoting, in place on the lower triangle) followed by solve(Identity), restated line
// for line as the reference uses it when Q_uu + lambda I is not PD on an unchecked step
// (src/Optimiser/iLQR.cpp:597-604); identical to generic.hip's dev_ldlt_inverse and oracle/orc_ldlt_inverse.
// M: m x m row-major with row stride ms; a, x: m*m work/result (column-major); temp: m; tr: m ints.
// Run by ONE lane; noinline with a run-time m so that the rare path costs no registers in the hot loop.
__device__ static __attribute__((noinline)) void kp_slow_ldlt_inverse(int m, const double *M, int ms, double *a, double *x, double *temp, int *tr)
{
#define AA(i, j) a[(i) + (j) * m]
#define XX(i, j) x[(i) + (j) * m]
    for (int j = 0; j < m; j++) for (int i = 0; i < m; i++) AA(i, j) = M[i * ms + j];
    for (int k = 0; k < m; k++) {
        int big = k; double bv = fabs(AA(k, k));
        for (int i = k + 1; i < m; i++) if (fabs(AA(i, i)) > bv) { bv = fabs(AA(i, i)); big = i; }
        tr[k] = big;
        if (big != k) {
            for (int j = 0; j < k; j++) { double t = AA(k, j); AA(k, j) = AA(big, j); AA(big, j) = t; }
            for (int i = big + 1; i < m; i++) { double t = AA(i, k); AA(i, k) = AA(i, big); AA(i, big) = t; }
            { double t = AA(k, k); AA(k, k) = AA(big, big); AA(big, big) = t; }
            for (int i = k + 1; i < big; i++) { double t = AA(i, k); AA(i, k) = AA(big, i); AA(big, i) = t; }
        }
        if (k > 0) {
            for (int j = 0; j < k; j++) temp[j] = AA(j, j) * AA(k, j);
            double dot = 0.0;
            for (int j = 0; j < k; j++) dot += AA(k, j) * temp[j];
            AA(k, k) -= dot;
            for (int i = k + 1; i < m; i++) {
                double d2 = 0.0;
                for (int j = 0; j < k; j++) d2 += AA(i, j) * temp[j];
                AA(i, k) -= d2;
            }
        }
        const double akk = AA(k, k);
        const bool valid = fabs(akk) > 0.0;
        if (k == 0 && !valid) { for (int j = 0; j < m; j++) tr[j] = j; break; }
        if (valid) for (int i = k + 1; i < m; i++) AA(i, k) /= akk;
    }
    for (int c = 0; c < m; c++) for (int r = 0; r < m; r++) XX(r, c) = (r == c) ? 1.0 : 0.0;
    for (int k = 0; k < m; k++)
        if (tr[k] != k) for (int c = 0; c < m; c++) { double t = XX(k, c); XX(k, c) = XX(tr[k], c); XX(tr[k], c) = t; }
    for (int c = 0; c < m; c++)
        for (int k = 0; k < m; k++) {
            const double b = XX(k, c);
            for (int i = k + 1; i < m; i++) XX(i, c) -= b * AA(i, k);
        }
    for (int i = 0; i < m; i++) {
        const double d = AA(i, i);
        for (int c = 0; c < m; c++) {
            if (fabs(d) > 2.2250738585072014e-308) XX(i, c) /= d; else XX(i, c) = 0.0;
        }
    }
    for (int c = 0; c < m; c++)
        for (int k = m - 1; k >= 0; k--) {
            const double b = XX(k, c);
            for (int i = 0; i < k; i++) XX(i, c) -= b * AA(k, i);
        }
    for (int k = m - 1; k >= 0; k--)
        if (tr[k] != k) for (int c = 0; c < m; c++) { double t = XX(k, c); XX(k, c) = XX(tr[k], c); XX(tr[k], c) = t; }
#undef AA
#undef XX
}

}  // namespace kpilqr
