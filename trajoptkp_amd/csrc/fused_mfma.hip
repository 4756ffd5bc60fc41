// fused_mfma.hip -- the "never materialise A, B, l_*" form of the backward (a7) and forward (a8) passes
// for n+2 <= 16: the interpolation of the dynamics Jacobians (a4) and the
// Gauss-Newton cost derivatives (a6) are evaluated INSIDE the two sweeps, from the differenced key-point columns in the
// key-point column store kpc [entry][3][n] (common.h: 3n doubles per (trajectory, DoF, key-point), no step records) and
// from the residuals / residual Jacobians.  The one-wave backward sweep also has a RAW form that differences the
// key-point ordered FD payload (x+ / x- in entry order, kpilqr_upload_fd_kp) itself at the segment crossings -- the
// arithmetic of Differentiator.cpp:166-222,441-457 -- and leaves kpc behind for the forward sweep: no differencing kernel,
// no intermediate pass over the payload.
//
//   * a4 (KeypointGenerator::InterpolateDerivatives, src/KeyPointGenerator/KeyPointGenerator.cpp:840-954):
//     in the MFMA "D" layout lane (c,q) holds rows 4r+q of COLUMN c of A (and of B), and the reference
//     interpolates column-wise with one key-point list per DoF -- so each lane walks the key-point list of
//     its own DoF and keeps (value at segment start, slope) in registers:
//         A_t[:,c] = A_s[:,c] + (t-s) * ((A_e[:,c] - A_s[:,c]) / (e-s))          (:898-905, :933-948)
//     the slope is the correctly rounded quotient k_interpolate forms; the value is ONE fused multiply-add of it
//     (lerp_nc: a single rounding where k_interpolate has two -- the sweeps are held to the oracle at 1e-9, the
//     materialised A, B of kpilqr_interpolate keep the reference's bits).  Key-point columns of the next segment are
//     fetched one segment ahead (time indices two ahead).
//   * a6 (ModelTranslator::CostDerivativesFromResiduals, src/ModelTranslator/ModelTranslator.cpp:552-583):
//     with Rz = [r_x | r] (nr x (n+1)) and W = diag(2w):  Lzz = [l_xx l_x; l_x' *] = Rz' W Rz is ONE
//     P(Rz, W Rz); l_uu and l_u come out of P(Ru, W [Ru | r]) (columns < m and column n).  The reference
//     has no l_ux term, so the cross product r_u' W r_x is never formed.  Terminal weights at t = T-1
//     (Optimiser::ComputeCostDerivatives, src/Optimiser/Optimiser.cpp:202-211).
//     The forward pass scores a candidate with the same model written on the residuals:
//         l_x'dx + dx'l_xx dx/2 = sum_k w_k Jx_k (2 r_k + Jx_k),   Jx = r_x dx      (likewise for du).
//
// Wave organisations (plan_backward_fused / plan_forward_fused pick by batch size):
//   backward: one wave per trajectory (batch > #SIMDs/2) | consumer / helper pair;
//   forward:  one wave -- in a form for uniform key-point sets (no LDS transpose) and a general one, chosen on the device --
//             | state / cost pair | state / cost / staging triple.
// Everything else (homogeneous form, LDL' solve, slow path, stores) is riccati_mfma.hip / forward_mfma.hip.
// Per launch the kernels read Kp*(n^2+nm) + T*nr*(1+n+m) doubles instead of T*(2n^2+nm+n+m^2+m).
#include <cstdlib>
#include <type_traits>
#include "mfma_common.h"

namespace kpilqr {

typedef unsigned long long u64;
#define BIGT 0x3fffffff
// An offset no trajectory's slice of kpc reaches (fused_supported keeps a slice below 1 GB): a lane / register / entry with
// nothing to load adds it instead of selecting -- BIGOFF and BIGOFF + BIGOFF are both out of range of the descriptor and do
// not wrap, so the load returns 0 (the store is dropped) without a compare-and-select per access.
#define BIGOFF 0x40000000

// Latency probe (-DKP_PROBE_SAMEB, tools/build_variant.sh): every workgroup of the one-wave sweeps works on one of eight
// trajectories, so all of its loads hit in cache -- the sweep time that is left is what the memory system does NOT account for
// (results are only meaningful for a batch that repeats 8 problems, synth.tile_problem).
#ifndef KP_FWD_SETS
#define KP_FWD_SETS 4              // register sets of the one-wave forward sweep (requests run this many steps ahead)
#endif
#ifndef KP_FWD_SETS_GEN
#define KP_FWD_SETS_GEN 6          // ... of its general (per-DoF list) form (late round 4, same box: 3 / 4 / 5 / 6 / 8 sets = 2.37 / 2.32 / 2.30 / 2.29 / 2.46 ms
                                   // on velocity_change lists, 2.73 / 2.70 / 2.65 / 2.64 / 2.81 on adaptive_jerk lists)
#endif
#ifndef KP_FSC_SETS
#define KP_FSC_SETS 4              // tile sets of the forward state / cost wave groups
#endif
#ifndef KP_PROBE_BWD
#define KP_PROBE_BWD 0
#endif
// The uniform one-wave backward sweeps symmetrise the Qzz tile IN FRONT of the refresh and take V' = Qs + K'G as it leaves the
// last product (ESYM in backward_fused_body).  0: V' symmetrised behind that product, as before (the A/B's other side).
// KP_EARLY_SYM_AT: where the transposed half is read -- 1 right behind the write, 2 behind the refresh, in front of the gains product.
#ifndef KP_EARLY_SYM
#define KP_EARLY_SYM 1
#endif
#ifndef KP_EARLY_SYM_AT
#define KP_EARLY_SYM_AT 1
#endif
// The launchers (and with them the kernel instantiations) of this file compile as THREE translation units (Makefile: -DKP_FUSED_PART=1|2|3;
// unset or 0: everything in one): 1 one wave per trajectory backward + the form choices, 2 the backward consumer / helper pair,
// 3 the forward sweeps -- the file takes two minutes as one unit.
#ifndef KP_FUSED_PART
#define KP_FUSED_PART 0
#endif
#define KP_PART(n) (KP_FUSED_PART == 0 || KP_FUSED_PART == (n))
#ifdef KP_PROBE_SAMEB
#define KP_BLOCK_TRAJ ((int)(blockIdx.x & 7))
#else
#define KP_BLOCK_TRAJ ((int)blockIdx.x)
#endif
// correctly rounded a/den for a normal-range quotient: one residual correction on top of a ~1 ulp reciprocal
// (the hardware division expansion without its scaling / fix-up tail; den is a small positive integer)
__device__ __forceinline__ double fdiv(double a, double den, double rinv)
{
    const double q0 = a * rinv;
    const double rr = __builtin_fma(-den, q0, a);
    return __builtin_fma(rr, rinv, q0);
}
// v_min_f64 / v_max_f64 as they are: the builtins come with a canonicalising v_max x, x, x of every operand under the IEEE mode
// of compute kernels -- per use, not hoisted -- which is what the clamp of the control law (iLQR.cpp:883-889) does NOT need: its
// limits are finite constants (a NaN candidate stays visible in the state and the predicted cost either way)
__device__ __forceinline__ double vmin64(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double vmax64(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double bits_or(double a, double b)
{
    return __builtin_bit_cast(double, __builtin_bit_cast(u64, a) | __builtin_bit_cast(u64, b));
}
__device__ __forceinline__ double bits_and(double a, u64 mask)
{
    return __builtin_bit_cast(double, __builtin_bit_cast(u64, a) & mask);
}
// start + dt*slope as ONE fused multiply-add (a single rounding where k_interpolate's un-contracted multiply and add have two:
// at least as close to the exact interpolant) -- 16 VALU instructions less per forward step and 8 per backward step on a wave that
// pays ~9 cycles for each; the sweeps' results move by ~1e-16 relative (they are held to the oracle at 1e-9, not bit for bit: the
// MFMA accumulation order differs from the reference's loops anyway); kpilqr_interpolate / get_AB still give the reference's bits.
__device__ __forceinline__ double lerp_nc(double sv, double dt, double av)
{
    return __builtin_fma(dt, av, sv);
}

struct FusedArgs {
    const int *kp_offsets, *kp_times;              // per (b, dof) CSR of key-point time indices
    const double *r, *r_x, *r_u, *w_run, *w_term;  // [b][T+1][nr], [..][nr][n], [..][nr][m], [nr], [nr]
    int dof, nr;
    double *kpc;                                   // key-point column store [entry][3][n] (read; written by the raw backward sweep)
    const char *fdk;                               // key-point ordered FD payload (raw backward sweep only): one record per entry,
                                                   // [(x+, x-) pairs of the 3n elements | int32 mode: bit k = kind k is one-sided | pad] = (6n + 2) * 8 bytes
    double eps2, rinv_2eps;                        // 2 eps and the host's correctly rounded 1 / (2 eps): with it fdiv IS the IEEE
                                                   // quotient (eps and 1/eps are exact halves / doubles of them)
    const double *rx_const;                        // RXC: r_x [nr][n], the same for every trajectory and step (kpilqr_upload_residual_jacobians_const)
    const double *kps;                             // slope store [entry][3][n][2] beside kpc: every key-point column with its slope to the
                                                   // next key-point of its DoF list (k_kp_slopes); read by the general (per-DoF list) forms
};

// ---- column tracker: lane (c,q) interpolates rows 4r+q of column c of A and of B ------------------------
// col[0..3] = A(4r+q, c), col[4..7] = B(4r+q, c) (c < m).  The whole trajectory's key-point columns -- entries
// [E0, E0 + NE) of kpc, 3n doubles each: position column | velocity column | control column of the entry's DoF -- sit
// behind one buffer descriptor; tk is the entry RELATIVE to E0 (anything outside [0, NE) reads zeros), and a lane with
// nothing to load carries an out-of-range offset and reads 0.
struct ColOffs { int a[4], b[4]; };

// offsets of lane (c, q) inside an entry: rows 4r+q of A column c (the position column of DoF c, or the velocity column of
// DoF c - dof) and of B column c
__device__ __forceinline__ void col_offsets(ColOffs &co, int n, int m, int dof, int c, int q)
{
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = 4 * r + q;
        co.a[r] = (row < n && c < n) ? 8 * ((c < dof ? 0 : n) + row) : BIGOFF;
        co.b[r] = (row < n && c < m) ? 8 * (2 * n + row) : BIGOFF;
    }
}

__device__ __forceinline__ void load_col(__amdgpu_buffer_rsrc_t rT, const ColOffs &o, int tk, int T, int strideB, double *col)
{
    const int base = ((unsigned)tk < (unsigned)T) ? tk * strideB : BIGOFF;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        col[r] = kp_bld(rT, base + o.a[r]);
        col[4 + r] = kp_bld(rT, base + o.b[r]);
    }
}

// (value, slope) pairs of the slope store kps [entry][3][n][2] (k_kp_slopes): ONE 16-byte load per element gives a segment's start
// value and its slope to the next key-point.  Offsets are those of kpc doubled.
__device__ __forceinline__ int dbl_off(int o) { return o == BIGOFF ? BIGOFF : 2 * o; }
__device__ __forceinline__ void load_col2(__amdgpu_buffer_rsrc_t rS, const ColOffs &o, int tk, int T, int strideB2, double *col, double *slp)
{
    const int base = ((unsigned)tk < (unsigned)T) ? tk * strideB2 : BIGOFF;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        kp_bld2(rS, base + dbl_off(o.a[r]), col[r], slp[r]);
        kp_bld2(rS, base + dbl_off(o.b[r]), col[4 + r], slp[4 + r]);
    }
}

// The same for a lane whose four registers are rows q, 4+q, 8+q, 12+q of ONE column (the column layout of the backward
// sweep): one offset per column and lane, the rows in the loads' immediate field.  Registers 4r+3 < N are valid in every
// lane that holds the column at all; the one partial register (N % 4 rows) has a per-lane offset of its own; registers
// beyond the column are zero without a load.
struct ColOffsN { int a, al, b, bl; };
template <int N>
__device__ __forceinline__ void col_offsets_n(ColOffsN &co, int m, int dof, int c, int q)
{
    constexpr int NF = N / 4;
    co.a = (c < N) ? 8 * ((c < dof ? 0 : N) + q) : BIGOFF;
    co.b = (c < m) ? 8 * (2 * N + q) : BIGOFF;
    co.al = (c < N && 4 * NF + q < N) ? 8 * ((c < dof ? 0 : N) + 4 * NF + q) : BIGOFF;
    co.bl = (c < m && 4 * NF + q < N) ? 8 * (2 * N + 4 * NF + q) : BIGOFF;
}
template <int N>
__device__ __forceinline__ void load_col_n(__amdgpu_buffer_rsrc_t rT, const ColOffsN &o, int base, double *col)
{
    constexpr int NF = N / 4;
    const int va = base + o.a, vb = base + o.b;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        col[r] = r < NF ? kp_bld(rT, va + 32 * r) : (r == NF && (N & 3)) ? kp_bld(rT, base + o.al) : 0.0;
        col[4 + r] = r < NF ? kp_bld(rT, vb + 32 * r) : (r == NF && (N & 3)) ? kp_bld(rT, base + o.bl) : 0.0;
    }
}
// (value, slope) pairs from the slope store, column layout (o2: col_offsets_n's offsets doubled)
template <int N>
__device__ __forceinline__ void load_col2_n(__amdgpu_buffer_rsrc_t rS, const ColOffsN &o2, int base2, double *col, double *slp)
{
    constexpr int NF = N / 4;
    const int va = base2 + o2.a, vb = base2 + o2.b;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (r < NF) { kp_bld2(rS, va + 64 * r, col[r], slp[r]); kp_bld2(rS, vb + 64 * r, col[4 + r], slp[4 + r]); }
        else if (r == NF && (N & 3)) { kp_bld2(rS, base2 + o2.al, col[r], slp[r]); kp_bld2(rS, base2 + o2.bl, col[4 + r], slp[4 + r]); }
        else { col[r] = 0.0; slp[r] = 0.0; col[4 + r] = 0.0; slp[4 + r] = 0.0; }
    }
}
template <int N>
__device__ __forceinline__ void store_col_n(__amdgpu_buffer_rsrc_t rT, const ColOffsN &o, int base, const double *col)
{
    constexpr int NF = N / 4;
    const int va = base + o.a, vb = base + o.b;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (r < NF) {
            kp_bst(col[r], rT, va + 32 * r);
            kp_bst(col[4 + r], rT, vb + 32 * r);
        } else if (r == NF && (N & 3)) {
            kp_bst(col[r], rT, base + o.al);
            kp_bst(col[4 + r], rT, base + o.bl);
        }
    }
}

// Every kernel of this file takes (RecLayout L, FusedArgs F, ...) first, so F sits at a fixed place of the kernel-argument
// segment.  Scalars that only a segment CROSSING needs (descriptors of the key-point stores, the key-point times, eps) are
// re-read from there inside the crossing -- scalar loads, every few steps -- instead of staying live across the hot loop,
// where the register allocator would park them in VGPR lanes and pay a v_readlane / v_writelane (a VALU slot each) per use.
static_assert(sizeof(RecLayout) == 40 && alignof(FusedArgs) == 8, "kernel-argument layout assumed by kernarg_fused()");
typedef const __attribute__((address_space(4))) FusedArgs *KArgF;
__device__ __forceinline__ KArgF kernarg_fused()
{
    const __attribute__((address_space(4))) char *ka = (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));                 // opaque: the loads below cannot be hoisted out of the loop that holds the call
    return (KArgF)(ka + 40);
}

// LDS of the backward kernel (doubles): the one-tile map of mfma_common.h
#define FLDS_TOTAL (KP_LDS_SLOW + 2 * 256 + 16 + 16)

// PC = false: one wavefront per trajectory does everything.  PC = true: this is the CONSUMER wave of the consumer / helper pair;
// the step's tiles Fu, [l_uu | l_u] (and Lzz of the terminal step) come from the LDS ring filled by the helper wave
// (fusedpc_producer below), which also forms the side products Quz, Qzz; two block barriers per step, mid-step and at its end.
#define FPC_TILES 4
#define FPC_BUF (FPC_TILES * 256)
// behind the two ring slots (offsets from the ring base): the helper wave's Quz and Qzz
#define FPC_SIDE_QUZ (2 * FPC_BUF)
#define FPC_SIDE_QZZ (FPC_SIDE_QUZ + 256)
// Quu + lambda I is not PD on an unchecked step: the pivoted inverse (one lane, kp_slow_ldlt_inverse) times Quz, as gains with their
// sign -- the tail of the inlined factorisation block of backward_fused_body, for the form whose factorisation is out of line.
template <int M>
__device__ __forceinline__ d4 kp_pivoted_gains(double *sh, int m_rt, int lane)
{
    constexpr int m = M;
    const int c = lane & 15, q = lane >> 4;
    double *wa = sh + KP_LDS_SLOW, *wx = wa + 256, *wt = wx + 256;
    int *tr = (int *)(wt + 16);
    if (lane == 0) kp_slow_ldlt_inverse(m_rt, sh + KP_LDS_Q, KP_MS, wa, wx, wt, tr);
    __builtin_amdgcn_wave_barrier();
    double x[M];
#pragma unroll
    for (int i = 0; i < M; i++) {
        double sacc = 0.0;
#pragma unroll
        for (int p = 0; p < M; p++) sacc += (-wx[i + p * m]) * sh[KP_LDS_Z + c * KP_MZ + p];
        x[i] = -sacc;
    }
    __builtin_amdgcn_wave_barrier();
    double xr[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < M; i++)
        if (q == (i & 3)) xr[i >> 2] = x[i];
    d4 Kp;
    Kp.x = -xr[0]; Kp.y = -xr[1]; Kp.z = -xr[2]; Kp.w = -xr[3];
    return Kp;
}

// The factorisation path of a step of the uniform one-wave sweep (the first step, checked steps, re-seeds: 1 % of the steps at the
// bench's pd_stride), OUT OF LINE: inlined, its ~100 live registers (Lm[M][M], rd, x, y) met the refreshed path at the join in front of
// the gains product, and the allocator parked Quz / Qr of EVERY refreshed step in AGPRs to make room for a branch that step does not
// take.  noinline like kp_slow_ldlt_inverse: what the rare path needs is saved and restored around the call, on the rare path.
// In: the LDS image of the step, Qr = Quu + lambda I at KP_LDS_Q and Quz' at KP_LDS_Z (written by the caller, wave barrier behind it).
// Out, in registers (2 NCU doubles and a word: a by-value aggregate of up to 16 registers comes back in VGPRs, a larger one through
// scratch): the lane's rows of the gains column with its sign, of the NEGATED inverse column, and the verdict.  A LEAF: the pivoted
// slow path stays with the caller (a call in here would have the return address saved in scratch).  The statements are the inlined
// block's, one for one: same arithmetic in the same order, same bits.
enum { KP_FACTOR_NOT_PD = 0, KP_FACTOR_SEEDED = 1, KP_FACTOR_INDEFINITE = 2 };   // checked step failed (:587-595) | LDL', Xinv seeded | unchecked, not PD: pivot
template <int NCU> struct FactorOut { double Kp[NCU], Xinv[NCU]; int verdict; };
template <int M>
__device__ static __attribute__((noinline)) FactorOut<(M + 3) / 4> kp_factor_path(const double *sh, int lane, bool check_pd)
{
    constexpr int m = M, NCU = (M + 3) / 4;
    static_assert(2 * 2 * NCU + 1 <= 16, "FactorOut must come back in registers");
    const int c = lane & 15, q = lane >> 4;
    FactorOut<NCU> o;
#pragma unroll
    for (int r = 0; r < NCU; r++) { o.Kp[r] = 0.0; o.Xinv[r] = 0.0; }
    // ---- unpivoted LDL' of Quu + lambda I, redundantly in every lane ----
    double Lm[M][M], rd[M];
    const bool pos = kp_ldl_factor<M>([&](int i, int j) { return sh[KP_LDS_Q + i * KP_MS + j]; }, Lm, rd);
    o.verdict = pos ? KP_FACTOR_SEEDED : check_pd ? KP_FACTOR_NOT_PD : KP_FACTOR_INDEFINITE;
    if (!pos) return o;
    double x[M];
#pragma unroll
    for (int i = 0; i < M; i++) x[i] = sh[KP_LDS_Z + c * KP_MZ + i];
    kp_ldl_solve<M>(Lm, rd, x);
    // seed the fast path: column c of the inverse in lane c (c < m), as a tile
    double y[M];
#pragma unroll
    for (int i = 0; i < M; i++) y[i] = (i == c) ? 1.0 : 0.0;
    kp_ldl_solve<M>(Lm, rd, y);
    double yr[NCU], xr[NCU];
#pragma unroll
    for (int r = 0; r < NCU; r++) { yr[r] = 0.0; xr[r] = 0.0; }
#pragma unroll
    for (int i = 0; i < M; i++)
        if (q == (i & 3)) { yr[i >> 2] = (c < m) ? y[i] : 0.0; xr[i >> 2] = x[i]; }
#pragma unroll
    for (int r = 0; r < NCU; r++) { o.Xinv[r] = -yr[r]; o.Kp[r] = -xr[r]; }       // the running inverse is kept negated
    return o;
}

// RU0: the context's r_u buffer was never written (a task without control residuals: r_u = 0, e.g. reaching,
// src/ModelTranslator/Reaching.cpp:43-54), so [l_uu | l_u] = Ru' W [Ru | r] is exactly zero: the product and the r_u loads
// are left out (4 of the step's 40 MFMAs).
// RAW (one wave per trajectory only): the sweep reads the key-point ordered FD payload (F.xp, F.xm, F.mode) instead of kpc,
// differences every column when it becomes a segment start -- (x+ - x-) / (2 eps), or / eps for a one-sided job, with
// the host's correctly rounded reciprocals, i.e. the bytes k_fd_kp_difference would write -- and stores it to kpc, which
// the forward sweep then reads.
// UNI (one wave per trajectory only): every DoF of the trajectory has the SAME key-point list (set_interval -- the reference's
// default -- and whatever else comes out uniform; the device flag of k_kp_uniform says so).  Segment start, end and position
// are then wave-uniform scalars, the sweep is a loop over SEGMENTS with the crossing in straight-line code at its top and the
// first step of the segment peeled behind it, and the loads of a crossing have a whole Riccati chain to land before anything
// waits for them.  (In the general form the crossing sits in a per-lane branch, behind which the compiler has to wait for
// every memory operation in flight at the next load-dependent instruction: ~1 us of HBM latency per crossing, 7.5 against
// 4.5 ms per sweep with a key-point at every step.)
// STATS (diagnostic instantiation, kpilqr_backward_stats): counts per trajectory what every step did to obtain
// (Quu + lambda I)^-1 -- hist[0] third-order refresh only, [1..3] plus that many second-order steps, [4] LDL' factorisation
// (first step, checked steps, re-seeds), [5] the pivoted slow path -- into hist [batch][6].
// RXC (one wave per trajectory, with RU0): the residual Jacobian r_x is the same [nr][n] matrix at every step of every
// trajectory (reaching: selector rows, src/ModelTranslator/Reaching.cpp:43-54; any task whose residuals are affine in the state):
// the Rx tile is loaded ONCE and stays in registers, the sweep issues no r_x loads (T nr n doubles per trajectory: 5.0 of the
// 8.1 MB a trajectory's backward sweep reads at the headline shape).  Same products in the same order: bit-identical gains.
template <int N, int M, bool PC, bool RU0 = false, bool RAW = false, bool UNI = false, bool STATS = false, bool RXC = false>
__device__ __forceinline__ void backward_fused_body(double *sh, const double *pcbuf, int *sflag, RecLayout L, FusedArgs F, int T,
                const double *__restrict__ lambda, int pd_stride, double *__restrict__ Kout, double *__restrict__ kout,
                double *__restrict__ delta_J, int *__restrict__ status, int *__restrict__ hist = nullptr, const int btraj = KP_BLOCK_TRAJ)
{
    int hcnt[6] = {0, 0, 0, 0, 0, 0};
    (void)hcnt;
    constexpr int NCZ = (N + 1 + 3) / 4;
    constexpr int NCU = (M + 3) / 4;
    constexpr int n = N, m = M;
    // HEADS (uniform one-wave sweeps): the rows behind 4 NCU of the running inverses and of the gains are not state -- Xh, Xq, Ksh are
    // the NCU live registers of Xinv, Xprev, Kst, and N0t is the tile whose head takes the extrapolated first guess of every step
    // (kp_inverse_refresh_heads); its zero tail is written here, once (opaque to the compiler, which would otherwise rebuild the tile
    // from a literal zero on every step).
    constexpr bool HEADS = UNI && !PC;
    double Xh[NCU], Xq[NCU], Ksh[NCU];
    double N0t[2] = {0.0, 0.0};
#pragma unroll
    for (int r = 0; r < NCU; r++) { Xh[r] = 0.0; Xq[r] = 0.0; Ksh[r] = 0.0; }
    // (Declared up here, in front of everything else: further down, beside the running inverse, these dead locals of the other forms
    // changed the order of the set-up code of the wave pairs' consumer -- two register pairs swapped in kernels that are not touched.
    // The tail is made opaque below, behind the set-up: see there.)
    (void)Xh; (void)Xq; (void)Ksh; (void)N0t;
    // one wavefront per workgroup (or the consumer wave of a group): its LDS operations execute in order, so a write ->
    // transposed read pair needs the compiler's ordering only (4.94 -> 4.87 ms against __syncthreads() in the one-wave forms).
    // (Tried: the transposed half requested at the end of a step and averaged in front of the next step's first Riccati
    // product, so that the LDS round trip runs under that step's a4 / a6 -- 7.73 ms: eight more live registers across the
    // top of the step.)
    auto wsync = [&]() { __builtin_amdgcn_wave_barrier(); };
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int b = btraj;                  // (the block's own index but in a listed launch: see k_backward_fused)
    const double lam = lambda[b];
    // (probe builds, -DKP_PROBE_BWD=bits: 1 residual loads, 2 key-point stores, 4 gain stores go to one of eight trajectories)
    const int bR = (KP_PROBE_BWD & 1) ? (int)(blockIdx.x & 7) : b, bP = (KP_PROBE_BWD & 2) ? (int)(blockIdx.x & 7) : b, bS = (KP_PROBE_BWD & 4) ? (int)(blockIdx.x & 7) : b;
    constexpr bool RV2B = RXC && RU0 && !PC;     // (see below)
    // 4-row chunks of the residual index that hold residuals (RV2B: registers 0, 1 hold residuals 0 .. 7, registers 2, 3 residuals 8 .. 15)
    const int nr = F.nr, ncr = RV2B ? (nr > 9 ? 4 : nr > 8 ? 3 : nr > 1 ? 2 : 1) : (nr + 3) >> 2;
    constexpr int strideB = 3 * N * 8;                            // bytes of one key-point entry: three columns

    ColOffsN co;
    col_offsets_n<N>(co, m, F.dof, c, q);
    double w2run[4], w2term[4], lam2d[4];
    int oRx[4], oR1[4], oRu[4], oKst[4], okst[4];
    // RV2B (the headline's one-wave sweep: constant r_x, no control residuals): the residuals sit in the rows of the Rz tiles in the order
    //     row 4r + q  <->  residual 8 (r >> 1) + 2 q + (r & 1)
    // -- registers (0, 1) and (2, 3) of a lane are consecutive residuals, so r_t arrives with two 16-byte requests instead of four
    // 8-byte ones (see RV2 in forward_fused_body).  The rows are the contraction index of every product they enter (Cxx, r_x' W r, the
    // terminal step's Rz' W Rz): a relabelling, with the weights relabelled alike.
    const int oR12[2] = {(2 * q < nr) ? 16 * q : KP_OOB, (8 + 2 * q < nr) ? 64 + 16 * q : KP_OOB};
    (void)oR12;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int kr = RV2B ? 8 * (r >> 1) + 2 * q + (r & 1) : 4 * r + q;     // the residual in row 4r + q
        oRx[r] = (kr < nr && c < n) ? 8 * (kr * n + c) : KP_OOB;        // Rz(k, c) = r_x[k][c]
        w2run[r] = (kr < nr) ? 2.0 * F.w_run[kr] : 0.0;
        w2term[r] = (kr < nr) ? 2.0 * F.w_term[kr] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = 4 * r + q;
        // (RXC one-wave sweeps: r[k] in EVERY column -- the lanes of column c form their part of (r_x' W r)(c) from it, see CXX below)
        oR1[r] = (row < nr && (c == n || (RXC && !PC))) ? 8 * row : KP_OOB;               //            ... | r[k] in column n
        oRu[r] = (row < nr && c < m) ? 8 * (row * m + c) : KP_OOB;      // Ru(k=row, c) = r_u[k][c]
        oKst[r] = (row < m && c < n) ? 8 * (row + c * m) : KP_OOB;
        okst[r] = (row < m && c == n) ? 8 * row : KP_OOB;
        lam2d[r] = (row == c && row < m) ? 2.0 * lam : 0.0;
    }
    const d4 LamI = {0.5 * lam2d[0], 0.5 * lam2d[1], 0.5 * lam2d[2], 0.5 * lam2d[3]};     // lambda on the diagonal of the u-block
    const u64 mask_n = (c == n) ? ~0ull : 0ull, mask_u = (c < m) ? ~0ull : 0ull;
    const bool lane_nn = (c == n) && (q == (n & 3));
    constexpr int REG_NN = n >> 2;

    // this trajectory's key-point entries [E0, E0 + NE): one descriptor over its slice of kpc (and of the raw payload)
    const int E0 = F.kp_offsets[(size_t)bP * F.dof], NE = F.kp_offsets[(size_t)(bP + 1) * F.dof] - E0;
    __amdgpu_buffer_rsrc_t rT = kp_rsrc(F.kpc + (size_t)E0 * 3 * n, NE * strideB);
    const double *rb = F.r + (size_t)bR * (T + 1) * nr;
    const double *rxb = F.r_x + (size_t)bR * (T + 1) * nr * n;
    const double *rub = F.r_u + (size_t)bR * (T + 1) * nr * m;

    struct ResTiles { d4 Rx, R1, Ru; };
    // The sweep asks for the steps in order (T-1, T-2, ...), so the three residual arrays and the two gain arrays are walked
    // with running pointers: a subtraction per array and step instead of a 64-bit (trajectory, step) product (-24 scalar
    // instructions per step, 4.84 -> 4.77 ms).  `t` only says whether there IS a step t (the general form asks once more at the bottom).
    const double *pRx = rxb + (size_t)(T - 1) * nr * n, *pR = rb + (size_t)(T - 1) * nr, *pRu = rub + (size_t)(T - 1) * nr * m;
    auto load_res = [&](int t, ResTiles &s) {
        __amdgpu_buffer_rsrc_t rR = kp_rsrc(pR, nr * 8);
        __amdgpu_buffer_rsrc_t rR2 = kp_rsrc(pR, nr * 8 + 8);
        (void)rR2;
        __amdgpu_buffer_rsrc_t rRu = kp_rsrc(pRu, nr * m * 8);
        if constexpr (!RXC) {
            __amdgpu_buffer_rsrc_t rRx = kp_rsrc(pRx, nr * n * 8);
            s.Rx.x = kp_bld(rRx, oRx[0]); s.Rx.y = kp_bld(rRx, oRx[1]); s.Rx.z = kp_bld(rRx, oRx[2]); s.Rx.w = kp_bld(rRx, oRx[3]);
            if (t > 0) pRx -= nr * n;
        }
        if (t > 0) { pR -= nr; pRu -= nr * m; }       // (behind step 0: stay on it)
        if constexpr (RV2B) {
            // (descriptor one element longer: the last pair of an odd residual count reaches into the next row -- the array has T + 1)
            double r0, r1, r2, r3;
            kp_bld2s(rR2, oR12[0], 0, r0, r1); kp_bld2s(rR2, oR12[1], 0, r2, r3);
            s.R1.x = r0; s.R1.y = r1; s.R1.z = r2; s.R1.w = r3;
        } else {
        s.R1.x = kp_bld(rR, oR1[0]); s.R1.y = kp_bld(rR, oR1[1]); s.R1.z = kp_bld(rR, oR1[2]); s.R1.w = kp_bld(rR, oR1[3]);
        }
        if constexpr (!RU0) { s.Ru.x = kp_bld(rRu, oRu[0]); s.Ru.y = kp_bld(rRu, oRu[1]); s.Ru.z = kp_bld(rRu, oRu[2]); s.Ru.w = kp_bld(rRu, oRu[3]); }
    };

    // ---- column tracker, walking DOWN in time ----------------------------------------------------------
    const int kd = (c < F.dof) ? c : c - F.dof;
    const bool has = !PC && c < n;
    const int lo = has ? F.kp_offsets[(size_t)bP * F.dof + kd] : 0;
    const int hi = has ? F.kp_offsets[(size_t)bP * F.dof + kd + 1] : 0;
    int idx = hi - 1;
    int s = has ? F.kp_times[idx] : -1;                       // == T-1 for canonical key-points
    int nb = (has && idx - 1 >= lo) ? F.kp_times[idx - 1] : -1;      // the time of the next segment start, one crossing ahead
    double sv[8], av[8], pv[8];
    // SLP (general form on a differenced column store): the SLOPE of the next segment is prefetched with its start column (pm),
    // from the slope store k_kp_slopes wrote -- a crossing is then two register moves per value, no division on the wave's
    // serial chain (8 correctly rounded divisions + a reciprocal per lane before: the whole wave paid them on every step on which
    // ANY lane crossed, which with per-DoF lists is most steps)
    constexpr bool SLP = !PC && !UNI && !RAW;
    // RAW: the prefetched column of the next segment start waits as x+ (in pv) and x- (pm) until the crossing differences it
    double pm[8];
    int pmode = 0;
    // the raw payload: ONE descriptor over the trajectory's records; x+ and x- of an element sit side by side (one 16-byte load
    // gives both: 9 loads per crossing instead of 17) and the mode word behind them
    constexpr int strideR = (6 * N + 2) * 8, offMode = 6 * N * 8;
    __amdgpu_buffer_rsrc_t rP = rT;                               // SLP: the trajectory's slice of the slope store: (value, slope) pairs
    ColOffsN co2 = co;
    co2.a = dbl_off(co.a); co2.al = dbl_off(co.al); co2.b = dbl_off(co.b); co2.bl = dbl_off(co.bl);
    auto ebase2 = [&](int e_rel) { return ((unsigned)e_rel < (unsigned)NE) ? e_rel * (2 * strideB) : BIGOFF; };
    (void)co2;
    if constexpr (SLP) rP = kp_rsrc(F.kps + (size_t)E0 * 6 * n, NE * 2 * strideB);
    const int bitA = (c < F.dof) ? 1 : 2;                         // mode bit of this lane's A column (position / velocity job)
    auto ebase = [&](int e_rel) { return ((unsigned)e_rel < (unsigned)NE) ? e_rel * strideB : BIGOFF; };
    auto load_raw = [&](int e_rel, double *xp_, double *xm_, int &mo) {
        const int base = ((unsigned)e_rel < (unsigned)NE) ? e_rel * strideR : BIGOFF;
        load_col2_n<N>(rP, co2, base, xp_, xm_);
        mo = __builtin_amdgcn_raw_buffer_load_b32(rP, base + ((c < n) ? offMode : BIGOFF), 0, 0);
    };
    double eps2 = F.eps2, rinv2 = F.rinv_2eps;
    auto difference_arith = [&](double *xp_, const double *xm_, int mo) {           // xp_ <- the differenced column
        // central differences are the rule (a control at its limit is the exception, Differentiator.cpp:94-143): one
        // wave-uniform test keeps the per-lane denominator selects off the usual path
        if (__builtin_amdgcn_ballot_w64(mo != 0) == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) xp_[i] = fdiv(xp_[i] - xm_[i], eps2, rinv2);
        } else {
            const bool oa = (mo & bitA) != 0, ob = (mo & 4) != 0;
            const double dA = oa ? 0.5 * eps2 : eps2, rA = oa ? 2.0 * rinv2 : rinv2;     // exact halves / doubles
            const double dB = ob ? 0.5 * eps2 : eps2, rB = ob ? 2.0 * rinv2 : rinv2;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                xp_[i] = fdiv(xp_[i] - xm_[i], dA, rA);
                xp_[4 + i] = fdiv(xp_[4 + i] - xm_[4 + i], dB, rB);
            }
        }
    };
    auto difference = [&](double *xp_, const double *xm_, int mo, int e_rel) {      // ... and out to kpc
        difference_arith(xp_, xm_, mo);
        store_col_n<N>(rT, co, ebase(e_rel), xp_);
    };
    (void)pm; (void)pmode; (void)bitA;
    ResTiles cur;
    // CXX (RXC, one wave per trajectory; round 5): with ONE r_x for every step, l_xx = r_x' W r_x IS THE SAME MATRIX at every step
    // below the terminal one (running weights) -- only l_x = r_x' W r moves.  The four dependent products of Lzz = Rz' W Rz become
    //     Lzz~ = Cxx + 2 e_n v',      v(c) = sum_k r_x[k][c] 2 w_k r[k]
    // ONE product: lane (c, q) adds up its four rows k = 4r + q on the VALU (p, four FMAs on the resident r_x W tile and a broadcast
    // load of r), and the sum over q IS the contraction of a 16x16x4 product whose first operand is 2 e_n in every k --
    // D(i, j) = sum_q 2 e_n(i) p(j, q) -- accumulated onto the resident tile Cxx.  Row n then carries 2 l_x and column n nothing:
    // Lzz~ only ever enters V' = Qzz + K'G, which the step symmetrises ((V' + V'')/2, iLQR.cpp:610), and (Lzz~ + Lzz~')/2 = Lzz
    // (element (n, n), the constant of the value function, is dropped by the sweep anyway).  The terminal step (V = Lzz under the
    // terminal weights, :537-539) keeps the full product.  31.4 matrix instructions per step instead of 34.4, and a chain of four at
    // the top of the step becomes one.  The accumulation order differs from the per-step form's: results agree to ~1e-15, not bit for bit.
    // (PACKQ, below: the same one product writes v into COLUMN n of the tile instead, see the step.)
    constexpr bool CXX = RXC && !PC;
    d4 Cxx = {0.0, 0.0, 0.0, 0.0}, RxW = Cxx;
    const double en2 = (c == n) ? 2.0 : 0.0, en1 = (c == n) ? 1.0 : 0.0;
    (void)Cxx; (void)RxW; (void)en2; (void)en1;
    if constexpr (RXC) {                           // the one r_x of the task: in registers for the whole sweep
        __amdgpu_buffer_rsrc_t rRx = kp_rsrc(F.rx_const, nr * n * 8);
        cur.Rx.x = kp_bld(rRx, oRx[0]); cur.Rx.y = kp_bld(rRx, oRx[1]); cur.Rx.z = kp_bld(rRx, oRx[2]); cur.Rx.w = kp_bld(rRx, oRx[3]);
        if constexpr (CXX) {
            RxW.x = cur.Rx.x * w2run[0]; RxW.y = cur.Rx.y * w2run[1]; RxW.z = cur.Rx.z * w2run[2]; RxW.w = cur.Rx.w * w2run[3];
            Cxx = kp_Pn(cur.Rx, RxW, Cxx, ncr);
        }
    }
    // UNI: lane offsets of the lane's own DoF list (kd * KpU entries into the slice), the position in the soffset operand
    const int KpU = F.kp_offsets[(size_t)bP * F.dof + 1] - E0;
    ColOffsN cu = co, cr = co;                                 // kpc / raw payload
    auto shift = [&](int v, int by) { return v == BIGOFF ? BIGOFF : v + by; };
    if constexpr (UNI) {
        cu.a = shift(co.a, kd * KpU * strideB); cu.al = shift(co.al, kd * KpU * strideB);
        cu.b = shift(co.b, kd * KpU * strideB); cu.bl = shift(co.bl, kd * KpU * strideB);
        cr.a = shift(co2.a, kd * KpU * strideR); cr.al = shift(co2.al, kd * KpU * strideR);      // (the payload's elements are 16 bytes)
        cr.b = shift(co2.b, kd * KpU * strideR); cr.bl = shift(co2.bl, kd * KpU * strideR);
    }
    // PACKQ (the uniform one-wave sweep at (14,7); n + 1 > 8, m <= 8): the tracker holds the two PACKED operand tiles of the step
    //     slot a: Y1 = [ Fz cols 0..7 | Fu in cols 8..8+m-1 | 0 ]        slot b: Pk = [ Fu | 0 (cols m..7) | Fz cols 8..n ]
    // -- lanes 8 .. 8+m-1 walk B column c - 8 (the list of DoF c - 8) in slot a and their own A column in slot b, which sat idle
    // in them; the per-lane offsets ride in the same load instructions, so a crossing issues no more requests.  The
    // duplicated B columns are not stored to kpc (cs).  See the products in `step`.
    constexpr bool PACKQ = UNI && !PC && N == 14 && M == 7;
    static_assert(!PACKQ || (N + 1 > 8 && M <= 8 && (M + 3) / 4 <= 2), "packed Q tiles: split row 8");
    // ESYM (uniform one-wave sweeps): of V' = Qzz + K'G only Qzz needs the transposition -- packed, its block rows 8.. x cols 0..7 is
    // never computed; with a constant r_x, l_x sits on one side of it -- and Qzz is complete in front of the refresh; K'G is a full
    // product, symmetric up to the rounding of its m terms.  So the tile goes through LDS right behind its product (packed: the merge),
    // Qs = Qm/2 + (Qm/2)' | (Qzz + Qzz')/2, off the chain V -> T2 -> D2 -> refresh -> K -> V', and V = Qs + K'G leaves the last product
    // as it is: no LDS round trip between the last product of a step and the first of the next.  V carries the rounding asymmetry of
    // ONE product (|V - V'| / |V| ~ 1e-16, tools/early_symmetrise_error.py); Qzz is symmetrised exactly at every step, so it does not
    // accumulate.  Measured at both placements of the read and on all four shapes: profiles/early_symmetrise.txt.
    constexpr bool ESYM = HEADS && KP_EARLY_SYM;
    auto esym_write = [&](const d4 &Q) {
        sh[KP_LDS_V + (q) * KP_VS + c] = Q.x;
        sh[KP_LDS_V + (4 + q) * KP_VS + c] = Q.y;
        sh[KP_LDS_V + (8 + q) * KP_VS + c] = Q.z;
        sh[KP_LDS_V + (12 + q) * KP_VS + c] = Q.w;
        wsync();
    };
    auto esym_read = [&](d4 &Q) {                              // Q <- Q + Q' (packed: the tile is halved) | (Q + Q')/2 on the image in KP_LDS_V
        Q.x += sh[KP_LDS_V + c * KP_VS + q];
        Q.y += sh[KP_LDS_V + c * KP_VS + 4 + q];
        Q.z += sh[KP_LDS_V + c * KP_VS + 8 + q];
        Q.w += sh[KP_LDS_V + c * KP_VS + 12 + q];
        if constexpr (!PACKQ) { Q.x *= 0.5; Q.y *= 0.5; Q.z *= 0.5; Q.w *= 0.5; }
        wsync();
    };
    (void)esym_write; (void)esym_read;
    ColOffsN cs = cu;                                          // raw sweep: where a differenced column goes in kpc
    (void)cs;
    if constexpr (PACKQ) {
        if (c >= 8) {
            constexpr int NF4 = 4 * (N / 4);
            const bool dup = c < 8 + m;
            const int jb = (c - 8) * KpU;
            const int b0 = 8 * (2 * N + q), bl0 = (NF4 + q < N) ? 8 * (2 * N + NF4 + q) : BIGOFF;
            ColOffsN bu, br;
            bu.a = dup ? b0 + jb * strideB : BIGOFF; bu.al = dup ? shift(bl0, jb * strideB) : BIGOFF;
            bu.b = cu.a; bu.bl = cu.al;
            br.a = dup ? 2 * b0 + jb * strideR : BIGOFF; br.al = dup ? shift(dbl_off(bl0), jb * strideR) : BIGOFF;
            br.b = cr.a; br.bl = cr.al;
            cs.a = BIGOFF; cs.al = BIGOFF; cs.b = cu.a; cs.bl = cu.al;
            cu = bu; cr = br;
        }
    }
    const bool lo8 = c < 8;
    (void)lo8;
    // PACKQ, the merge: the cost block Lzz joins the merged tile of V' = Qm + K'G by FMAs on per-lane constants instead of riding in the
    // initial values of the D products, and the tile is formed HALVED, so that V = acc + acc' below needs no 0.5:
    //     Qm/2 = f o D + L/2,     f = 1/2 in the blocks (rows, cols) < 8 and >= 8, 1 in rows < 8 x cols >= 8 (it stands for its never
    //     computed mirror image too), 0 in that mirror image; L/2 is the whole symmetric cost block halved (its two halves add up).
    // The 0 factor needs a finite D there: that block of D2 is a product of the same finite operands as the blocks that are read.
    // Halving is exact (a power of two; V' of a sweep is nowhere near 2^-1021, where the halves of normal numbers stop being exact).
    const double f_lo = lo8 ? 0.5 : 1.0, f_hi = lo8 ? 0.0 : 0.5;
    const d4 Cxxh = {0.5 * Cxx.x, 0.5 * Cxx.y, 0.5 * Cxx.z, 0.5 * Cxx.w};
    (void)f_lo; (void)f_hi; (void)Cxxh;
    int up = KpU - 1;                                          // UNI: position (in every list) of the current segment's start
    int us = T, unb = T - 1, unb_v = T - 1;                    // UNI: its time, and the time of the next start (uniform; unb_v: as loaded)
    (void)up; (void)us; (void)unb; (void)unb_v; (void)cu; (void)cr;
    if constexpr (!PC && UNI) {
        // both columns of the first crossing are the last key-point's (slope 0 over the virtual segment [T-1, T])
        if constexpr (RAW) {
            rP = kp_rsrc(F.fdk + (size_t)E0 * strideR, NE * strideR);
            load_col2_n<N>(rP, cr, up * strideR, pv, pm);
            pmode = __builtin_amdgcn_raw_buffer_load_b32(rP, up * strideR + kd * KpU * strideR + ((c < n) ? offMode : BIGOFF), 0, 0);
#pragma unroll
            for (int i = 0; i < 8; i++) sv[i] = 0.0;
        } else {
            load_col_n<N>(rT, cu, up * strideB, pv);
#pragma unroll
            for (int i = 0; i < 8; i++) sv[i] = pv[i];
        }
#pragma unroll
        for (int i = 0; i < 8; i++) av[i] = 0.0;
        load_res(T - 1, cur);
    } else if constexpr (!PC) {
        const int e_s = has ? idx - E0 : -1, e_nb = (has && idx - 1 >= lo) ? idx - 1 - E0 : -1;
        if constexpr (RAW) {
            rP = kp_rsrc(F.fdk + (size_t)E0 * strideR, NE * strideR);
            int mo0;
            load_raw(e_s, sv, pm, mo0);
            difference(sv, pm, mo0, e_s);
            load_raw(e_nb, pv, pm, pmode);
        } else {
            load_col_n<N>(rT, co, ebase(e_s), sv);
            load_col2_n<N>(rP, co2, ebase2(e_nb), pv, pm);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) av[i] = 0.0;
        // Fz(n,n) = 1: lane c == n walks no list (never crosses), so its constant start value carries the 1
#pragma unroll
        for (int r = 0; r < 4; r++) if (c == n && 4 * r + q == n) sv[r] = 1.0;
        // single-buffered: the residual tiles are consumed by the first MFMAs of a step and re-requested for the
        // next step right behind them (a whole step of latency cover, no register copies)
        load_res(T - 1, cur);
    } else {
        __syncthreads();                               // the producer has published step T-1
    }
    // HEADS: the tail of the first-guess tile becomes opaque HERE, behind the set-up.  In front of it (beside the declarations) the
    // statement made the compiler treat the set-up's descriptors (E0, rT) as per-lane values in the job-list (kpc) forms: a
    // readfirstlane loop around every crossing's loads (tools/isa_lint.py: waterfall loops).
    if constexpr (HEADS) asm volatile("" : "+v"(N0t[0]), "+v"(N0t[1]));
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    d4 V = zero, accp = zero;                                  // accp (PC): V' of the step before, not yet symmetrised
    (void)accp;
    // (PACKQ: behind the terminal step W2 holds HALF the running weights -- the cost block of the merge is formed halved -- and the
    // [l_uu | l_u] product of a sweep with control residuals doubles it back, exactly.  Every other form: the running weights.)
    d4 W2 = {w2term[0], w2term[1], w2term[2], w2term[3]};     // terminal weights at t = T-1, running after
    int pd_counter = 0, fail = 0;
    double dJ = 0.0;
    d4 Xinv = zero, Xprev = zero, Iu;            // running inverse of Quu + lambda I, the one before it, the identity of the u-block
    bool haveX = false;
    Iu.x = (q == c && c < m) ? 1.0 : 0.0; Iu.y = (4 + q == c && c < m) ? 1.0 : 0.0;
    Iu.z = (8 + q == c && c < m) ? 1.0 : 0.0; Iu.w = (12 + q == c && c < m) ? 1.0 : 0.0;
    (void)haveX; (void)Iu;

    // The gains of a step leave the wave one step late (one-wave forms), in front of the next residual requests: a wait
    // for those requests also waits for every store issued behind them (the counter is shared and in order), and stores
    // issued at the end of a step are acknowledged by a loaded memory system long after the requests have come back --
    // the wait at the top of every step sat out that acknowledgement.  In front of the requests the stores are a step old
    // when anything waits for them.
    d4 Kst = zero;
    int tst = -1, kst_pos = -1;
    (void)Kst; (void)tst; (void)kst_pos;
    double *pK = Kout + ((size_t)bS * T + T - 1) * m * n, *pk = kout + ((size_t)bS * T + T - 1) * m;
    auto store_gains = [&](int t, const d4 &Kp) {
        (void)t;                                       // the steps are stored in order, T-1 first
        __amdgpu_buffer_rsrc_t rK = kp_rsrc(pK, m * n * 8);
        __amdgpu_buffer_rsrc_t rk = kp_rsrc(pk, m * 8);
        pK -= m * n; pk -= m;
        const double kv[4] = {Kp.x, Kp.y, Kp.z, Kp.w};
#pragma unroll
        for (int r = 0; r < NCU; r++) {
            kp_bst(kv[r], rK, oKst[r]);
            kp_bst(kv[r], rk, okst[r]);
        }
    };
    // one step of the sweep; false: the PD check of this step failed (the sweep ends)
#ifdef KP_CYC
    unsigned long long cyc_cross = 0, cyc_peel = 0, cyc_inner = 0, cyc_a = 0, cyc_b = 0, cyc_c = 0, cyc_d = 0, cyc_e = 0;
    const unsigned long long cyc_all0 = __builtin_readcyclecounter();
#endif
    // may_be_first: whether this call site can see the terminal step t = T-1 (only the first step of a sweep can: the call
    // sites inside the loops say no, and the selects of the terminal value function and weights leave the hot path)
    auto step = [&](int t, auto may_be_first) __attribute__((always_inline)) -> bool {
#ifdef KP_CYC
        const unsigned long long cyc_s0 = __builtin_readcyclecounter();
#endif
        d4 Fz, Fu, Lzz, LU;
        d4 Lh = zero;                                  // PACKQ: Lzz / 2
        (void)Lh;
        d4 Y1 = zero;                                  // PACKQ: the packed tile of slot a
        (void)Y1;
        const bool term = decltype(may_be_first)::value && (t == T - 1);
        bool cross = false;                            // general form: this lane has crossed the start of its segment
        (void)cross;
        if constexpr (PC) {
            const double *tb = pcbuf + (t & 1) * FPC_BUF;
            Fu = kp_lds_tile(tb + 256, lane);
            if constexpr (RU0) LU = zero; else LU = kp_lds_tile(tb + 768, lane);
            // Fz, Lzz are the helper wave's operands; only V = Lzz of the last step is ours
            Fz = zero; Lzz = zero;
            if (term) Lzz = kp_lds_tile(tb + 512, lane);
            else {
                // (V' + V'')/2 of the step before: its transposed half is read here, behind the barrier that ended that
                // step, together with this step's tiles -- no write / wait / read round trip at the end of a step
                V.x = 0.5 * (accp.x + sh[KP_LDS_V + c * KP_VS + q]);
                V.y = 0.5 * (accp.y + sh[KP_LDS_V + c * KP_VS + 4 + q]);
                V.z = 0.5 * (accp.z + sh[KP_LDS_V + c * KP_VS + 8 + q]);
                V.w = 0.5 * (accp.w + sh[KP_LDS_V + c * KP_VS + 12 + q]);
                if (lane_nn) kp_set_reg<REG_NN>(V, 0.0);
            }
        } else {
        // ---- a4: this step's A and B columns --------------------------------------------------------------
        // General form (per-lane lists): a lane that has crossed the start of its segment takes the column prefetched a
        // crossing ago as the new start and forms the slope -- arithmetic only up here.  Everything of the crossing that is
        // a memory operation (the differenced column out to kpc, the next column and its time in) waits for `late_cross`
        // below, BEHIND the wait for this step's residual tiles: in front of it the wait, which the compiler has to place
        // conservatively behind a divergent branch, drained the requests the branch had just issued -- a trip to HBM on
        // every step on which any lane crossed (ragged key-point sets: most steps; 8.89 -> 8.32 and 9.61 -> 8.72 ms on two such sets).
        if constexpr (!UNI) {
            cross = t < s;
            if (cross) {
                if constexpr (SLP) {
                    // the new segment [nb, s): its start column and its slope were requested a crossing ago
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        asm volatile("v_mov_b64 %0, %1" : "+v"(av[i]) : "v"(pm[i]));
                        asm volatile("v_mov_b64 %0, %1" : "+v"(sv[i]) : "v"(pv[i]));
                    }
                } else {                              // RAW: the slope is formed here
                const KArgF Fk = kernarg_fused(); eps2 = Fk->eps2; rinv2 = Fk->rinv_2eps;
                const double den = (double)(s - nb);
                const double rinv = kp_rcp(den);
                difference_arith(pv, pm, pmode);        // the prefetched x+ / x- become the column
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    av[i] = fdiv(sv[i] - pv[i], den, rinv);
                    // a real move, in sv's own register: left to the compiler, sv is renamed onto pv's register, the loads below
                    // land somewhere else, and the two arrays are copied back and forth -- behind a wait for every memory
                    // operation in flight -- on EVERY step of the sweep instead of at the crossings
                    asm volatile("v_mov_b64 %0, %1" : "+v"(sv[i]) : "v"(pv[i]));
                }
                }
                idx--;
                s = nb;
            }
        }
        const double dt = UNI ? (double)(t - us) : (double)(t - s);
        Fz.x = lerp_nc(sv[0], dt, av[0]); Fz.y = lerp_nc(sv[1], dt, av[1]);
        Fz.z = lerp_nc(sv[2], dt, av[2]); Fz.w = lerp_nc(sv[3], dt, av[3]);
        Fu.x = lerp_nc(sv[4], dt, av[4]); Fu.y = lerp_nc(sv[5], dt, av[5]);
        Fu.z = lerp_nc(sv[6], dt, av[6]); Fu.w = lerp_nc(sv[7], dt, av[7]);
        Y1 = Fz;                                        // PACKQ: slot a is Y1, slot b (Fu) is Pk; Fz is the per-lane pick
        if constexpr (PACKQ) { Fz.x = lo8 ? Y1.x : Fu.x; Fz.y = lo8 ? Y1.y : Fu.y; Fz.z = lo8 ? Y1.z : Fu.z; Fz.w = lo8 ? Y1.w : Fu.w; }
        // ---- a6: Lzz, l_uu, l_u from the residuals --------------------------------------------------------
        if constexpr (CXX) {
            if (term) {                                 // (compile-time false away from a sweep's first step)
                d4 Rz;
                Rz.x = bits_or(cur.Rx.x, bits_and(cur.R1.x, mask_n)); Rz.y = bits_or(cur.Rx.y, bits_and(cur.R1.y, mask_n));
                Rz.z = bits_or(cur.Rx.z, bits_and(cur.R1.z, mask_n)); Rz.w = bits_or(cur.Rx.w, bits_and(cur.R1.w, mask_n));
                Lzz = kp_Pn(Rz, Rz * W2, zero, ncr);
            } else {
                double p = RxW.x * cur.R1.x;
                p = __builtin_fma(RxW.y, cur.R1.y, p); p = __builtin_fma(RxW.z, cur.R1.z, p); p = __builtin_fma(RxW.w, cur.R1.w, p);
                if constexpr (PACKQ) {
                    // packed Q products (below): of row n the merged Qzz tile keeps columns 8.. only, so v goes into COLUMN n instead
                    // (p as the first operand: D(i, n) = sum_q p(i, q)), once, on the halved constant block: (L/2)(i, n) = v(i),
                    // (L/2)(n, i) = 0, and their sum is l_x.  Still one product, up here off the Riccati chain.  (Tried: the product behind
                    // the merge, C = the merged tile, so that only the lane sums live across the top of the step -- it lost:
                    // it sits in the chain in front of the refresh, profiles/inner_step_moves_ab.txt.)
                    Lzz = KP_MFMA(p, en1, Cxxh);
                }
                else Lzz = KP_MFMA(en2, p, Cxx);
            }
        } else {
        d4 Rz;
        Rz.x = bits_or(cur.Rx.x, cur.R1.x); Rz.y = bits_or(cur.Rx.y, cur.R1.y);
        Rz.z = bits_or(cur.Rx.z, cur.R1.z); Rz.w = bits_or(cur.Rx.w, cur.R1.w);
        Lzz = kp_Pn(Rz, Rz * W2, zero, ncr);
        }
        if constexpr (PACKQ) {
            // the halved cost block of the merge.  A sweep's first step wants Lzz whole as well (V = Lzz): halved there, by four
            // multiplies on that one step; below it the tile is formed halved (Cxxh; W2 holds the halved running weights).
            if (term) { Lh.x = 0.5 * Lzz.x; Lh.y = 0.5 * Lzz.y; Lh.z = 0.5 * Lzz.z; Lh.w = 0.5 * Lzz.w; }
            else Lh = Lzz;
        }
        if constexpr (RU0) {
            LU = zero;
        } else {
            d4 Rur;
            Rur.x = bits_or(cur.Ru.x, cur.R1.x); Rur.y = bits_or(cur.Ru.y, cur.R1.y);
            Rur.z = bits_or(cur.Ru.z, cur.R1.z); Rur.w = bits_or(cur.Ru.w, cur.R1.w);
            if (PACKQ && !term) LU = kp_Pn(cur.Ru, Rur * (W2 + W2), zero, ncr);      // ([l_uu | l_u] under the whole running weights)
            else LU = kp_Pn(cur.Ru, Rur * W2, zero, ncr);
        }
        __builtin_amdgcn_sched_barrier(0);
        // the step above, IN FRONT of the requests.  (The test is false only at the first step; compiling it out of the loops'
        // call sites was measured and is 0.04 ms SLOWER at B=1024 -- the scheduler's placement of the stores changes.)
        if constexpr (HEADS) {
            d4 Ka = zero;
            Ka.x = Ksh[0]; if constexpr (NCU > 1) Ka.y = Ksh[1];
            if (tst >= 0) store_gains(tst, Ka);
        } else
        if (tst >= 0) store_gains(tst, Kst);
        if constexpr (!UNI) {
            if (cross) {                               // late_cross: the memory operations of the crossing at the top of this step
                const KArgF Fk = kernarg_fused();      // crossing-only scalars, from the kernel-argument segment
                rT = kp_rsrc(Fk->kpc + (size_t)E0 * 3 * n, NE * strideB);
                if constexpr (RAW) {
                    rP = kp_rsrc(Fk->fdk + (size_t)E0 * strideR, NE * strideR);
                    store_col_n<N>(rT, co, ebase(idx - E0), sv);          // the column that has just become the start value
                }
                nb = (idx - 1 >= lo) ? Fk->kp_times[idx - 1] : -1;
                const int e_nb = (idx - 1 >= lo) ? idx - 1 - E0 : -1;
                if constexpr (RAW) load_raw(e_nb, pv, pm, pmode);
                else {
                    rP = kp_rsrc(Fk->kps + (size_t)E0 * 6 * n, NE * 2 * strideB);
                    load_col2_n<N>(rP, co2, ebase2(e_nb), pv, pm);             // start column AND slope of the next segment: one load each
                }
            }
        }
        if constexpr (RAW && UNI) {
            // the differenced column of the crossing above (it is the segment's start value now): like the gains it leaves
            // behind the wait for this step's tiles -- in front of it, the wait sat out the stores' acknowledgement
            if (kst_pos >= 0) { store_col_n<N>(rT, cs, kst_pos * strideB, sv); kst_pos = -1; }
        }
        // (unconditional: a request behind `if (t > 0)` costs a scalar branch per step and makes the compiler's later waits
        // conservative -- in the general form its wait for the crossing's columns drained the tiles; 4.76 -> 4.70 ms in the
        // uniform form.  Behind step 0 the request repeats step 0's tiles, never used.)
        load_res(t > 0 ? t - 1 : 0, cur);
        __builtin_amdgcn_sched_barrier(0);
#ifdef KP_CYC
        cyc_a += __builtin_readcyclecounter() - cyc_s0;
#endif
        }
        d4 Luu, Luz;
        Luu.x = bits_and(LU.x, mask_u); Luu.y = bits_and(LU.y, mask_u); Luu.z = bits_and(LU.z, mask_u); Luu.w = bits_and(LU.w, mask_u);
        Luz.x = bits_and(LU.x, mask_n); Luz.y = bits_and(LU.y, mask_n); Luz.z = bits_and(LU.z, mask_n); Luz.w = bits_and(LU.w, mask_n);
        if (term) {                                     // V_x = l_x[T-1]; V_xx = l_xx[T-1]   (iLQR.cpp:537-539)
            V = Lzz;
            W2.x = w2run[0]; W2.y = w2run[1]; W2.z = w2run[2]; W2.w = w2run[3];
            if constexpr (PACKQ) { W2.x *= 0.5; W2.y *= 0.5; W2.z *= 0.5; W2.w *= 0.5; }       // (Lzz / 2 of the steps below: see Lh)
        }
        pd_counter++;
        const bool check_pd = pd_counter >= pd_stride;

        // ---- Tu = V' Fu ; Quu = l_uu + Fu' Tu --------------------------------------- :577
        // (one wave per trajectory: the regularisation rides in the accumulator's initial value, Qr = (l_uu + lambda I) + Fu'Tu -- nothing
        // downstream wants the un-regularised Quu: V' and delta_J are written on Qr, G and lambda below -- so the adds leave the chain
        // behind the product: 4.15 -> 4.10 ms at B=1024.  The consumer wave of the pair measured 1 % SLOWER with it and keeps the adds.)
        d4 Qr, Quz, Qzz;
        if constexpr (PACKQ) {
            // Quu, Quz and every needed entry of Qzz from TWO products on the packed tiles instead of three (16 matrix instructions
            // instead of 20): Fu' Tu fills 7 x 7 and Fu' Tz 7 x 15 of a 16 x 16 output, and Qzz is symmetric like the V' it enters.
            //     T2 = V' Pk = [Tu | 0 | Tz cols 8..n]
            //     D2 = Pk' T2: rows / cols < m are Quu, rows / cols 8..n are Qzz[8:, 8:], the rest is never read
            //     D1 = Y1' Tz: rows 0..7 are Qzz[0:8, :], rows 8..8+m-1 are Quz
            // The split row 8 is a register pair: (.x, .y) <-> (.z, .w) is a renaming.  The accumulators start from the cost terms of
            // the blocks that are read.  Qr = D2 goes to the refresh as it is: column 7 of Pk is zero, columns 8.. of Qr only make
            // rows >= 8 of the residual, which NCU = 2 never reads, and the LDL' path reads elements (i, j) < m.
            const d4 T2 = kp_P<NCZ>(V, Fu, zero);          // (first: the per-lane pick of Fz lands under it)
            const d4 Tz = kp_P<NCZ>(V, Fz, zero);
            // Lzz enters nothing but V' (Luz, Luu are rows < m of the u-block): it joins at the merge, and the accumulators start from
            // what the gains need -- without control residuals the resident lambda I (its rows 8.. are zero: m <= 8) and literal zero:
            // no register is moved to assemble a C operand
            d4 i2 = LamI, i1 = zero;
            if constexpr (!RU0) { i2.x = Luu.x + LamI.x; i2.y = Luu.y + LamI.y; i1.z = Luz.x; i1.w = Luz.y; }
            const d4 D2 = kp_P<NCZ>(Fu, T2, i2);
            const d4 D1 = kp_P<NCZ>(Y1, Tz, i1);
            Qr = D2;
            Quz.x = D1.z; Quz.y = D1.w; Quz.z = 0.0; Quz.w = 0.0;
            // the merge (f_lo, f_hi above): four FMAs on constants, Qm / 2
            Qzz.x = __builtin_fma(D1.x, f_lo, Lh.x); Qzz.y = __builtin_fma(D1.y, f_lo, Lh.y);
            Qzz.z = __builtin_fma(D2.z, f_hi, Lh.z); Qzz.w = __builtin_fma(D2.w, f_hi, Lh.w);
        } else {
        const d4 Tu = kp_P<NCZ>(V, Fu, zero);
        Qr = kp_P<NCZ>(Fu, Tu, PC ? Luu : Luu + LamI);          // Quu (+ lambda I)
        if constexpr (PC) { Qr.x += LamI.x; Qr.y += LamI.y; Qr.z += LamI.z; Qr.w += LamI.w; }
        // ---- Tz, Quz, Qzz --------------------------------------------------------------- :570-579
        if constexpr (PC) {
            Quz = zero; Qzz = zero;                   // the helper wave forms them meanwhile: read behind the refresh
        } else {
            d4 Tz = kp_P<NCZ>(V, Fz, zero);
            Quz = kp_P<NCZ>(Fu, Tz, Luz);
            Qzz = kp_P<NCZ>(Fz, Tz, Lzz);
        }
        }
        if constexpr (ESYM) {                          // Qs, in Qzz's registers
            esym_write(Qzz);
            if constexpr (KP_EARLY_SYM_AT == 1) esym_read(Qzz);
        }
#ifdef KP_CYC
        asm volatile("" :: "v"(Qr.x), "v"(Quz.x), "v"(Qzz.x));
        const unsigned long long cyc_s1 = __builtin_readcyclecounter();
        cyc_b += cyc_s1 - cyc_s0;
#endif

        // ---- X = (Quu + lambda I)^-1 Quz.  Fast path: the inverse changes little from one step to the next,
        //      so it is refreshed by Newton-Schulz steps Xinv <- Xinv + Xinv (I - Q Xinv) on the matrix core (4 MFMAs
        //      each, quadratic convergence; the count is chosen from the measured residual so that it ends below
        //      1e-15) and X = Xinv Quz is one more product -- the reference, too, forms the explicit inverse and
        //      multiplies (iLQR.cpp:597-604).  The LDL' path below runs on the first step, on every checked step
        //      (it gives the PD verdict of :587-595), and whenever the residual is too large to converge fast.
        bool done = false;
        int ns_steps = 0;
        // (segment-loop forms: the peeled step is the one right below a key-point -- known at compile time; which steps are peeled,
        // the re-seed below and its Xprev = Xinv are mirrored in tests/_refresh.py)
        constexpr bool KINK = UNI && !PC && decltype(may_be_first)::value;
        bool refreshed;                                 // Xinv, Xprev (HEADS: Xh, Xq): NEGATED inverses
        if constexpr (HEADS) refreshed = haveX && !check_pd && kp_inverse_refresh_heads<NCU, KINK>(Qr, Iu, N0t, Xh, Xq, m, STATS ? &ns_steps : nullptr);
        else refreshed = haveX && !check_pd && kp_inverse_refresh_n<NCU, KINK, PC>(Qr, Iu, Xinv, Xprev, m, STATS ? &ns_steps : nullptr);
        if constexpr (STATS) { if (refreshed) hcnt[ns_steps < 0 ? 0 : ns_steps > 3 ? 3 : ns_steps]++; }
        if constexpr (PC) {                           // mid-step barrier of the pair: Quz, Qzz are published
            __syncthreads();
            Quz = kp_lds_tile(pcbuf + FPC_SIDE_QUZ, lane); Qzz = kp_lds_tile(pcbuf + FPC_SIDE_QZZ, lane);
        }
#ifdef KP_CYC
        asm volatile("" :: "v"(Xinv.x));
        const unsigned long long cyc_s2 = __builtin_readcyclecounter();
        cyc_c += cyc_s2 - cyc_s1;
#endif
        if constexpr (ESYM && KP_EARLY_SYM_AT == 2) esym_read(Qzz);      // (in front of the factor path's LDS images too)
        d4 Kp = zero;                                 // the gains -X
        if (refreshed) {
            d4 Xa = Xinv;
            if constexpr (HEADS) { Xa = zero; Xa.x = Xh[0]; if constexpr (NCU > 1) Xa.y = Xh[1]; }     // (the product reads the NCU heads)
            Kp = kp_P<NCU>(Xa, Quz, zero);                 // -(Quu + lambda I)^-1 Quz: the gains, with their sign
            done = true;
        }
        if (!done) {
            sh[KP_LDS_Q + q * KP_MS + c] = Qr.x;
            if (NCU > 1) sh[KP_LDS_Q + (4 + q) * KP_MS + c] = Qr.y;
            if (NCU > 2) sh[KP_LDS_Q + (8 + q) * KP_MS + c] = Qr.z;
            if (NCU > 3) sh[KP_LDS_Q + (12 + q) * KP_MS + c] = Qr.w;
            sh[KP_LDS_Z + c * KP_MZ + q] = Quz.x;
            if (NCU > 1) sh[KP_LDS_Z + c * KP_MZ + 4 + q] = Quz.y;
            if (NCU > 2) sh[KP_LDS_Z + c * KP_MZ + 8 + q] = Quz.z;
            if (NCU > 3) sh[KP_LDS_Z + c * KP_MZ + 12 + q] = Quz.w;
            wsync();
            if constexpr (UNI && !PC) {                // out of line: the refreshed path keeps its registers (kp_factor_path)
                const FactorOut<NCU> fo = kp_factor_path<M>(sh, lane, check_pd);
                // every lane factorises the same broadcast image: one verdict.  Inlined, the compiler saw that (loads at a uniform
                // address); a value back from a call is per-lane to it, and through haveX every branch of the step became an EXEC-mask
                // region (4.61 against 4.00 ms).  Said here instead.
                const int verdict = __builtin_amdgcn_readfirstlane(fo.verdict);
                if (verdict == KP_FACTOR_NOT_PD) { fail = t + 1; return false; }
                if (check_pd) pd_counter = 0;
                haveX = verdict == KP_FACTOR_SEEDED;
                if (haveX) {
                    double kr[4] = {-0.0, -0.0, -0.0, -0.0}, yr[4] = {-0.0, -0.0, -0.0, -0.0};     // (rows behind NCU: as the negated zeros of the inlined form)
#pragma unroll
                    for (int r = 0; r < NCU; r++) { kr[r] = fo.Kp[r]; yr[r] = fo.Xinv[r]; }
                    Kp.x = kr[0]; Kp.y = kr[1]; Kp.z = kr[2]; Kp.w = kr[3];
                    if constexpr (HEADS) {
#pragma unroll
                        for (int r = 0; r < NCU; r++) { Xh[r] = fo.Xinv[r]; Xq[r] = fo.Xinv[r]; }      // re-seed: heads only
                    } else {
                    Xinv.x = yr[0]; Xinv.y = yr[1]; Xinv.z = yr[2]; Xinv.w = yr[3];
                    Xprev = Xinv;
                    }
                } else {
                    Kp = kp_pivoted_gains<M>(sh, L.m, lane);
                }
            } else {
            // ---- unpivoted LDL' of Quu + lambda I, redundantly in every lane ----
            double Lm[M][M], rd[M];
            const bool pos = kp_ldl_factor<M>([&](int i, int j) { return sh[KP_LDS_Q + i * KP_MS + j]; }, Lm, rd);
            if (check_pd) {                       // CheckMatrixPD every pd_stride steps   :587-595
                if (!pos) {
                    fail = t + 1;
                    if (PC) { if (lane == 0) sflag[0] = fail; __syncthreads(); }      // the producer leaves with us
                    return false;
                }
                pd_counter = 0;
            }
            double x[M];
            if (pos) {
#pragma unroll
                for (int i = 0; i < M; i++) x[i] = sh[KP_LDS_Z + c * KP_MZ + i];
                kp_ldl_solve<M>(Lm, rd, x);
                // seed the fast path: column c of the inverse in lane c (c < m), as a tile
                double y[M];
#pragma unroll
                for (int i = 0; i < M; i++) y[i] = (i == c) ? 1.0 : 0.0;
                kp_ldl_solve<M>(Lm, rd, y);
                double yr[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int i = 0; i < M; i++)
                    if (q == (i & 3)) yr[i >> 2] = (c < m) ? y[i] : 0.0;
                Xinv.x = -yr[0]; Xinv.y = -yr[1]; Xinv.z = -yr[2]; Xinv.w = -yr[3];       // the running inverse is kept negated
                Xprev = Xinv;
                haveX = true;
                if constexpr (STATS) hcnt[4]++;
            } else {
                if constexpr (STATS) hcnt[5]++;
                double *wa = sh + KP_LDS_SLOW, *wx = wa + 256, *wt = wx + 256;
                int *tr = (int *)(wt + 16);
                if (lane == 0) kp_slow_ldlt_inverse(L.m, sh + KP_LDS_Q, KP_MS, wa, wx, wt, tr);
                wsync();
#pragma unroll
                for (int i = 0; i < M; i++) {
                    double sacc = 0.0;
#pragma unroll
                    for (int p = 0; p < M; p++) sacc += (-wx[i + p * m]) * sh[KP_LDS_Z + c * KP_MZ + p];
                    x[i] = -sacc;
                }
                wsync();
                haveX = false;
            }
            double xr[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < M; i++)
                if (q == (i & 3)) xr[i >> 2] = x[i];
            Kp.x = -xr[0]; Kp.y = -xr[1]; Kp.z = -xr[2]; Kp.w = -xr[3];
            }
        }
        if constexpr (HEADS) { Ksh[0] = Kp.x; if constexpr (NCU > 1) Ksh[1] = Kp.y; tst = t; }
        else if constexpr (!PC) { Kst = Kp; tst = t; }
        else store_gains(t, Kp);
        // delta_J += k'Q_u + k'Q_uu k = -lambda k'k (:612-613): lanes of column n keep the squares of their rows,
        // the four row groups are added once after the sweep
        // (every lane accumulates; only the lanes of column n are read behind the sweep)
        // (the squares are summed, -lambda joins behind the sweep: one FMA per register and step)
        dJ = __builtin_fma(Kp.x, Kp.x, dJ);
        if (NCU > 1) dJ = __builtin_fma(Kp.y, Kp.y, dJ);
        if (NCU > 2) dJ = __builtin_fma(Kp.z, Kp.z, dJ);
        if (NCU > 3) dJ = __builtin_fma(Kp.w, Kp.w, dJ);
        // V' = Qzz + K'Quu K + K'Quz + Quz'K (:606-607) with K = -X, (Quu + lambda I) X = Quz:
        //    = Qzz - X'(Quz + lambda X) = Qzz + K'(Quz - lambda K)   -- one product; G = (Quu + 2 lambda I)K' is never formed
        // (PACKQ: Qzz is the merged tile Qm / 2 -- the block rows 8..n x cols 0..7 is never computed, its mirror image counts twice -- and
        // acc + acc' below gives every entry of V what it was, up to the summation order.  ESYM: Qzz is Qs by now, symmetric and whole.)
        d4 G;
        if constexpr (PACKQ && ESYM) {                   // Qzz is Qs, whole: G whole, on the NCU = 2 live registers
            G.x = __builtin_fma(-lam, Kp.x, Quz.x); G.y = __builtin_fma(-lam, Kp.y, Quz.y);
            G.z = 0.0; G.w = 0.0;
        } else if constexpr (PACKQ) {                    // G / 2 for the halved tile: NCU = 2 registers enter the product
            G.x = __builtin_fma(-0.5 * lam, Kp.x, 0.5 * Quz.x); G.y = __builtin_fma(-0.5 * lam, Kp.y, 0.5 * Quz.y);
            G.z = 0.0; G.w = 0.0;
        } else {
        G.x = __builtin_fma(-lam, Kp.x, Quz.x); G.y = __builtin_fma(-lam, Kp.y, Quz.y);
        G.z = __builtin_fma(-lam, Kp.z, Quz.z); G.w = __builtin_fma(-lam, Kp.w, Quz.w);
        }
        d4 acc = kp_P<NCU>(Kp, G, Qzz);
#ifdef KP_CYC
        asm volatile("" :: "v"(acc.x));
        const unsigned long long cyc_s3 = __builtin_readcyclecounter();
        cyc_d += cyc_s3 - cyc_s2;
#endif
        if constexpr (ESYM) {                          // V' as the product leaves it: nothing between it and the next step's T2
            V = acc;
            if (lane_nn) kp_set_reg<REG_NN>(V, 0.0);
        } else {
        sh[KP_LDS_V + (q) * KP_VS + c] = acc.x;
        sh[KP_LDS_V + (4 + q) * KP_VS + c] = acc.y;
        sh[KP_LDS_V + (8 + q) * KP_VS + c] = acc.z;
        sh[KP_LDS_V + (12 + q) * KP_VS + c] = acc.w;
        if constexpr (PC) {
            accp = acc;                                // symmetrised at the top of the next step, by this wave and by the helper wave
        } else {
            wsync();
            if constexpr (PACKQ) {                     // acc is V' / 2
                V.x = acc.x + sh[KP_LDS_V + c * KP_VS + q];
                V.y = acc.y + sh[KP_LDS_V + c * KP_VS + 4 + q];
                V.z = acc.z + sh[KP_LDS_V + c * KP_VS + 8 + q];
                V.w = acc.w + sh[KP_LDS_V + c * KP_VS + 12 + q];
            } else {
            V.x = 0.5 * (acc.x + sh[KP_LDS_V + c * KP_VS + q]);
            V.y = 0.5 * (acc.y + sh[KP_LDS_V + c * KP_VS + 4 + q]);
            V.z = 0.5 * (acc.z + sh[KP_LDS_V + c * KP_VS + 8 + q]);
            V.w = 0.5 * (acc.w + sh[KP_LDS_V + c * KP_VS + 12 + q]);
            }
            if (lane_nn) kp_set_reg<REG_NN>(V, 0.0);
        }
        if (PC) __syncthreads();                       // end of step: the ring slot is free, the next one is full
        else wsync();
        }
#ifdef KP_CYC
        asm volatile("" :: "v"(V.x));
        cyc_e += __builtin_readcyclecounter() - cyc_s3;
#endif
        return true;
    };
    if constexpr (UNI && !PC) {
        // (Tried: ONE loop over the steps with the crossing's arithmetic behind a uniform branch at the top of the step and its
        // memory operations behind the tile wait, as in the forward sweep and in the general form -- 5.64 against 4.81 ms, also
        // with a key-point every 20 steps (5.20 against 4.41): the loop as a whole came out slower, not the crossing.)
        // segments from the top: [k_p, k_p+1) with k_KpU := T.  The crossing -- slope of the new segment from the column
        // prefetched a segment ago, the next column requested (raw: x+ / x- differenced and kept for the forward sweep) --
        // is straight-line code; the segment's first step is peeled behind it so that the wait for its residual tiles
        // (requested BEFORE the crossing's loads) can leave those in flight.
        bool ok = true;
        for (; up >= 0 && ok; up--) {
#ifdef KP_CYC
            const unsigned long long cyc0 = __builtin_readcyclecounter();
#endif
            const KArgF Fk = kernarg_fused();                      // crossing-only scalars, from the kernel-argument segment
            rT = kp_rsrc(Fk->kpc + (size_t)E0 * 3 * n, NE * strideB);
            if constexpr (RAW) { rP = kp_rsrc(Fk->fdk + (size_t)E0 * strideR, NE * strideR); eps2 = Fk->eps2; rinv2 = Fk->rinv_2eps; }
            // the time of the new segment's start was requested a crossing ago, BEHIND that crossing's column loads: memory
            // operations return in order, and the wait for the residual tiles of the peeled step ("all but the youngest
            // loads") would otherwise have to sit out this load's latency too (measured: +840 cycles on every peeled step)
            unb = __builtin_amdgcn_readfirstlane(unb_v);
            const int gap = us - unb;                              // steps of the new segment (k_p+1 - k_p; 1 for the first)
            const double den = (double)gap, rinv = kp_rcp(den);
            if constexpr (RAW) {
                if (__builtin_amdgcn_ballot_w64(pmode != 0) == 0) {
#pragma unroll
                    for (int i = 0; i < 8; i++) pv[i] = fdiv(pv[i] - pm[i], eps2, rinv2);
                } else {
                    bool oa = (pmode & bitA) != 0, ob = (pmode & 4) != 0;
                    if constexpr (PACKQ) {
                        // lanes 8 ..: slot a is the control column of DoF c - 8 (its mode word sits in lane c - 8), slot b the lane's A column
                        const int m8 = __shfl(pmode, (lane - 8) & 63);
                        if (!lo8) { ob = oa; oa = (m8 & 4) != 0; }
                    }
                    const double dA = oa ? 0.5 * eps2 : eps2, rA = oa ? 2.0 * rinv2 : rinv2;     // exact halves / doubles
                    const double dB = ob ? 0.5 * eps2 : eps2, rB = ob ? 2.0 * rinv2 : rinv2;
#pragma unroll
                    for (int i = 0; i < 4; i++) { pv[i] = fdiv(pv[i] - pm[i], dA, rA); pv[4 + i] = fdiv(pv[4 + i] - pm[4 + i], dB, rB); }
                }
                kst_pos = up;                                      // stored from sv behind the tile wait of the step below
                if (up == KpU - 1) {
#pragma unroll
                    for (int i = 0; i < 8; i++) sv[i] = pv[i];
                }
            }
#pragma unroll
            for (int i = 0; i < 8; i++) { av[i] = fdiv(sv[i] - pv[i], den, rinv); sv[i] = pv[i]; }
            if (c == n) {                                          // Fz(n,n) = 1 rides in the idle lane's constant start value
#pragma unroll
                for (int r = 0; r < 4; r++) if (4 * r + q == n) { sv[(PACKQ ? 4 : 0) + r] = 1.0; av[(PACKQ ? 4 : 0) + r] = 0.0; }
            }
            const int t_hi = us - 1;
            us = unb;
            const int pn = up > 0 ? up - 1 : 0;                    // the next start (position 0 again at the bottom: never used)
            if constexpr (RAW) {
                load_col2_n<N>(rP, cr, pn * strideR, pv, pm);
                pmode = __builtin_amdgcn_raw_buffer_load_b32(rP, pn * strideR + kd * KpU * strideR + ((c < n) ? offMode : BIGOFF), 0, 0);
            } else {
                load_col_n<N>(rT, cu, pn * strideB, pv);
            }
            __builtin_amdgcn_sched_barrier(0);
            unb_v = Fk->kp_times[E0 + pn];                         // behind the column loads (see above)
            __builtin_amdgcn_sched_barrier(0);
#ifdef KP_CYC
            const unsigned long long cyc1 = __builtin_readcyclecounter();
            cyc_cross += cyc1 - cyc0;
#endif
            ok = step(t_hi, std::true_type{});                     // peeled: straight-line behind the crossing
#ifdef KP_CYC
            const unsigned long long cyc2 = __builtin_readcyclecounter();
            cyc_peel += cyc2 - cyc1;
#endif
            for (int t = t_hi - 1; t >= us && ok; t--) ok = step(t, std::false_type{});
#ifdef KP_CYC
            cyc_inner += __builtin_readcyclecounter() - cyc2;
#endif
        }
    } else {
        if (step(T - 1, std::true_type{}))
            for (int t = T - 2; t >= 0; t--) if (!step(t, std::false_type{})) break;
    }
    if constexpr (HEADS) { Kst.x = Ksh[0]; if constexpr (NCU > 1) Kst.y = Ksh[1]; }      // (heads of the last completed step)
    if constexpr (!PC) { if (tst >= 0) store_gains(tst, Kst); }      // the last completed step
    dJ *= -lam;
    dJ += __shfl_xor(dJ, 16);
    dJ += __shfl_xor(dJ, 32);
    if (lane_nn) delta_J[b] = dJ;
#ifdef KP_CYC
    if (lane_nn) { delta_J[b] = (double)cyc_cross; Kout[(size_t)b * T * m * n] = (double)cyc_peel; Kout[(size_t)b * T * m * n + 1] = (double)cyc_inner;
                   Kout[(size_t)b * T * m * n + 2] = (double)(__builtin_readcyclecounter() - cyc_all0); Kout[(size_t)b * T * m * n + 3] = (double)cyc_a;
                   Kout[(size_t)b * T * m * n + 4] = (double)cyc_b; Kout[(size_t)b * T * m * n + 5] = (double)cyc_c;
                   Kout[(size_t)b * T * m * n + 6] = (double)cyc_d; Kout[(size_t)b * T * m * n + 7] = (double)cyc_e; }
#endif
    if (lane == 0) status[b] = fail;
    if constexpr (STATS) {
        if (lane == 0) for (int i = 0; i < 6; i++) hist[(size_t)b * 6 + i] = hcnt[i];
    }
}

template <int N, int M>
__global__ void __launch_bounds__(64)
k_backward_fused_stats(RecLayout L, FusedArgs F, int T, const double *__restrict__ lambda,
                       int pd_stride, double *__restrict__ Kout, double *__restrict__ kout,
                       double *__restrict__ delta_J, int *__restrict__ status, int *__restrict__ hist)
{
    __shared__ __attribute__((aligned(16))) double sh[FLDS_TOTAL];
    backward_fused_body<N, M, false, false, false, false, true>(sh, nullptr, nullptr, L, F, T, lambda, pd_stride, Kout, kout, delta_J, status, hist);
}

// The one-wave backward sweep comes in two forms, launched back to back like the forward sweep's: UNI for key-point sets in
// which every DoF of a trajectory has the same list, the general form otherwise; each looks at the device flag first and
// leaves if the set is not its kind.
// EXCL, GATED: the trailing flags of every backward sweep kernel (riccati_mfma.hip says why a wave wants a SIMD to
// itself).  GATED runs the attempts behind the first of a backward pass under a lambda retry schedule (kpilqr_set_lambda_retry,
// lambda_retry.hip): a wave whose trajectory is settled or has given up (gate[b] == 0) leaves before anything else; the first
// attempt, and every launch without a schedule, is GATED = false, which reads neither `gate` nor `list`.
// GATED also runs the sweeps of a listed subset (kpilqr_backward_partial): `list` (device, nullptr: every block sweeps its own index)
// names the trajectory of block i, gate and every per-trajectory address follow it, and the caller has armed the gate of the listed
// trajectories.  list[blockIdx.x] is a scalar load off a kernel argument: the index stays wave-uniform, as the descriptors need it.
template <int N, int M, bool RU0, bool RAW, bool UNI, bool RXC, bool EXCL, bool GATED>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, EXCL ? 1 : 0)))
k_backward_fused(RecLayout L, FusedArgs F, int T, const double *__restrict__ lambda,
                 int pd_stride, double *__restrict__ Kout, double *__restrict__ kout,
                 double *__restrict__ delta_J, int *__restrict__ status, const int *__restrict__ kp_uniform, const int *__restrict__ gate,
                 const int *__restrict__ list)
{
    __shared__ __attribute__((aligned(16))) double sh[FLDS_TOTAL];
    const int b = GATED ? kp_block_traj(list, KP_BLOCK_TRAJ) : KP_BLOCK_TRAJ;
    if constexpr (GATED) { if (gate[b] == 0) return; }
    if ((*kp_uniform != 0) != UNI) return;
    backward_fused_body<N, M, false, RU0, RAW, UNI, false, RXC>(sh, nullptr, nullptr, L, F, T, lambda, pd_stride, Kout, kout, delta_J, status, nullptr, b);
}

// ---------------------------------------------------------------------------------------------------------
// Column trackers of the helper wave (consumer / helper pair below): a4 walking DOWN in time, NV values per lane.
template <int NV>
__device__ __forceinline__ void load_vals(__amdgpu_buffer_rsrc_t rT, const int *offs, int tk, int T, int strideB, double *out)
{
    const int base = ((unsigned)tk < (unsigned)T) ? tk * strideB : BIGOFF;
#pragma unroll
    for (int r = 0; r < NV; r++) out[r] = kp_bld(rT, base + offs[r]);
}

// Column tracker walking down for NV values per lane (a4), shared by the two roles.  (The list walk -- lo, idx, s, nb, nb2 -- is repeated in the two trackers below on purpose: profiles/mfma_primitives_isa.txt, 3.)
template <int NV>
struct DownTracker {
    int offs[NV];
    int lo, idx, s, nb, nb2;
    double sv[NV], av[NV], pv[NV];
    // rT: the trajectory's slice of kpc, entries [E0, E0 + NE) of strideB bytes each (see load_col)
    int E0, NE;
    __device__ __forceinline__ void init(__amdgpu_buffer_rsrc_t rT, const int *kp_offsets, const int *kp_times, bool has, size_t list, int E0_, int NE_, int strideB)
    {
        E0 = E0_; NE = NE_;
        lo = has ? kp_offsets[list] : 0;
        const int hi = has ? kp_offsets[list + 1] : 0;
        idx = hi - 1;
        s = has ? kp_times[idx] : -1;
        nb = (has && idx - 1 >= lo) ? kp_times[idx - 1] : -1;
        nb2 = (has && idx - 2 >= lo) ? kp_times[idx - 2] : -1;
        load_vals<NV>(rT, offs, has ? idx - E0 : -1, NE, strideB, sv);
        load_vals<NV>(rT, offs, (has && idx - 1 >= lo) ? idx - 1 - E0 : -1, NE, strideB, pv);
#pragma unroll
        for (int i = 0; i < NV; i++) av[i] = 0.0;
    }
    // a crossing in two halves: its arithmetic, and -- behind the wave's wait for
    // its residual tiles -- the request of the next column (a wait placed behind the divergent branch is conservative and would
    // sit out requests issued in front of it)
    bool need = false;
    __device__ __forceinline__ void cross(int t)
    {
        need = t < s;
        if (need) {
            const double den = (double)(s - nb);
            const double rinv = kp_rcp(den);
#pragma unroll
            for (int i = 0; i < NV; i++) {
                const double ev = sv[i];
                sv[i] = pv[i];
                av[i] = fdiv(ev - sv[i], den, rinv);
            }
            s = nb; idx--;
            nb = nb2;
        }
    }
    __device__ __forceinline__ void request(__amdgpu_buffer_rsrc_t rT, const int *kp_times, int strideB)
    {
        if (need) {
            nb2 = (idx - 2 >= lo) ? kp_times[idx - 2] : -1;
            load_vals<NV>(rT, offs, (idx - 1 >= lo) ? idx - 1 - E0 : -1, NE, strideB, pv);
        }
    }
    __device__ __forceinline__ double value(int i, double dt) const { return lerp_nc(sv[i], dt, av[i]); }
};

// The same on the SLOPE STORE (kps [entry][3][n][2], (value, slope) pairs: k_kp_slopes / k_fd_kp_difference<SLOPES>) -- per-DoF lists
// in the helper wave of the consumer / helper pair: a crossing is register moves and 16-byte loads, no division (with the lists of
// reaching.yaml's velocity_change some lane crosses on ~40 % of the steps).  The requests are issued by ALL lanes behind a
// wave-uniform branch (a lane that did not cross asks again for the entry it holds): loads inside a per-lane branch meet the
// old values at its join, and the wait the compiler places there drains every request in flight.
struct DownTrackerSlp {
    static constexpr int NV = 8;
    int offs[NV];                                // byte offsets inside a kpc entry (doubled for the slope store)
    int lo, idx, s, nb, nb2;
    double sv[NV], av[NV], pv[NV], pa[NV];
    int E0, NE;
    bool need = false;
    __device__ __forceinline__ void load_pairs(__amdgpu_buffer_rsrc_t rS, int e_rel, int stride2, double *v, double *a) const
    {
        const int base = ((unsigned)e_rel < (unsigned)NE) ? e_rel * stride2 : BIGOFF;
#pragma unroll
        for (int r = 0; r < NV; r++) kp_bld2(rS, base + dbl_off(offs[r]), v[r], a[r]);
    }
    __device__ __forceinline__ void init(__amdgpu_buffer_rsrc_t rS, const int *kp_offsets, const int *kp_times, bool has, size_t list, int E0_, int NE_, int stride2)
    {
        E0 = E0_; NE = NE_;
        lo = has ? kp_offsets[list] : 0;
        const int hi = has ? kp_offsets[list + 1] : 0;
        idx = hi - 1;
        s = has ? kp_times[idx] : -1;
        nb = (has && idx - 1 >= lo) ? kp_times[idx - 1] : -1;
        nb2 = (has && idx - 2 >= lo) ? kp_times[idx - 2] : -1;
        load_pairs(rS, has ? idx - E0 : -1, stride2, sv, av);                     // (the last key-point's slope is 0)
        load_pairs(rS, (has && idx - 1 >= lo) ? idx - 1 - E0 : -1, stride2, pv, pa);
    }
    __device__ __forceinline__ void cross(int t)
    {
        need = t < s;                            // per lane: crossed the start of the current segment
        if (need) {
#pragma unroll
            for (int i = 0; i < NV; i++) { sv[i] = pv[i]; av[i] = pa[i]; }
            s = nb; idx--;
            nb = nb2;
        }
    }
    __device__ __forceinline__ void request(__amdgpu_buffer_rsrc_t rS, const int *kp_times, int stride2)
    {
        if (__builtin_amdgcn_ballot_w64(need) != 0) {
            nb2 = (idx - 2 >= lo) ? kp_times[idx - 2] : -1;
            load_pairs(rS, (idx - 1 >= lo) ? idx - 1 - E0 : -1, stride2, pv, pa);
        }
    }
    __device__ __forceinline__ double value(int i, double dt) const { return lerp_nc(sv[i], dt, av[i]); }
};

// The same walking the KEY-POINT ORDERED FD PAYLOAD (helper wave of the pair, RAWP): the prefetched x+ / x- of the
// next segment start are differenced when the lane reaches it -- (x+ - x-) / (2 eps), / eps for a one-sided job: the arithmetic
// and the bytes of k_fd_kp_difference -- and the column goes out to kpc for the forward sweep.  The helper is a step ahead of the
// consumer and not the longer wave: the differencing costs the sweep nothing (a streaming kernel in front of it: 0.09 ... 0.41 ms
// at 128 ... 512 trajectories).  Values 0..3 of a lane belong to its A column (kind 0 / 1), 4..7 to its B column (kind 2).
struct DownTrackerRaw {
    static constexpr int NV = 8;
    int offs[NV];
    int lo, idx, s, nb, nb2, pmode, bitA;
    double sv[NV], av[NV], pv[NV], pm[NV];
    int E0, NE, strideR, offMode, strideB;
    bool has, fresh;                             // fresh: pv / pm still hold x+ / x- (not differenced yet)
    __device__ __forceinline__ void load_raw(__amdgpu_buffer_rsrc_t rP, int e_rel, double *xp, double *xm, int &mo) const
    {
        const int base = ((unsigned)e_rel < (unsigned)NE) ? e_rel * strideR : BIGOFF;
#pragma unroll
        for (int r = 0; r < NV; r++) kp_bld2(rP, base + dbl_off(offs[r]), xp[r], xm[r]);      // (x+, x-) of an element: one 16-byte load
        mo = __builtin_amdgcn_raw_buffer_load_b32(rP, base + (has ? offMode : BIGOFF), 0, 0);
    }
    __device__ __forceinline__ void diff(double *xp, const double *xm, int mo, double eps2, double rinv2) const
    {
        const bool oa = (mo & bitA) != 0, ob = (mo & 4) != 0;
        const double dA = oa ? 0.5 * eps2 : eps2, rA = oa ? 2.0 * rinv2 : rinv2;     // exact halves / doubles
        const double dB = ob ? 0.5 * eps2 : eps2, rB = ob ? 2.0 * rinv2 : rinv2;
#pragma unroll
        for (int i = 0; i < 4; i++) { xp[i] = fdiv(xp[i] - xm[i], dA, rA); xp[4 + i] = fdiv(xp[4 + i] - xm[4 + i], dB, rB); }
    }
    __device__ __forceinline__ void store(__amdgpu_buffer_rsrc_t rT, int e_rel, const double *x) const
    {
        const int base = ((unsigned)e_rel < (unsigned)NE) ? e_rel * strideB : BIGOFF;
#pragma unroll
        for (int r = 0; r < NV; r++) kp_bst(x[r], rT, base + offs[r]);
    }
    __device__ __forceinline__ void init(__amdgpu_buffer_rsrc_t rT, __amdgpu_buffer_rsrc_t rP, const int *kp_offsets, const int *kp_times, bool has_,
                                         size_t list, int E0_, int NE_, int n, bool pos_col, double eps2, double rinv2)
    {
        E0 = E0_; NE = NE_; has = has_;
        strideB = 3 * n * 8; strideR = (6 * n + 2) * 8; offMode = 6 * n * 8;
        bitA = pos_col ? 1 : 2;
        lo = has ? kp_offsets[list] : 0;
        const int hi = has ? kp_offsets[list + 1] : 0;
        idx = hi - 1;
        s = has ? kp_times[idx] : -1;
        nb = (has && idx - 1 >= lo) ? kp_times[idx - 1] : -1;
        nb2 = (has && idx - 2 >= lo) ? kp_times[idx - 2] : -1;
        int mo0;
        load_raw(rP, has ? idx - E0 : -1, sv, pm, mo0);
        diff(sv, pm, mo0, eps2, rinv2);
        store(rT, has ? idx - E0 : -1, sv);
        load_raw(rP, (has && idx - 1 >= lo) ? idx - 1 - E0 : -1, pv, pm, pmode);
        fresh = has && idx - 1 >= lo;                // (nothing below the list's first key-point: nothing to difference or store)
#pragma unroll
        for (int i = 0; i < NV; i++) av[i] = 0.0;
    }
    // the prefetched x+ / x- differenced (and stored) as soon as they have arrived -- a step behind their request, on a step
    // that has time for it -- so that the crossing itself is left with the slopes and the next requests
    __device__ __forceinline__ void settle(__amdgpu_buffer_rsrc_t rT, double eps2, double rinv2)
    {
        if (fresh) {
            diff(pv, pm, pmode, eps2, rinv2);
            store(rT, idx - 1 - E0, pv);
            fresh = false;
        }
    }
    bool need = false;
    __device__ __forceinline__ void cross(__amdgpu_buffer_rsrc_t rT, int t, double eps2, double rinv2)
    {
        need = t < s;
        if (need) {
            const double den = (double)(s - nb);
            const double rinv = kp_rcp(den);
            settle(rT, eps2, rinv2);
#pragma unroll
            for (int i = 0; i < NV; i++) {
                const double ev = sv[i];
                sv[i] = pv[i];
                av[i] = fdiv(ev - sv[i], den, rinv);
            }
            s = nb; idx--;
            nb = nb2;
        }
    }
    __device__ __forceinline__ void request(__amdgpu_buffer_rsrc_t rP, const int *kp_times)
    {
        if (need) {
            nb2 = (idx - 2 >= lo) ? kp_times[idx - 2] : -1;
            load_raw(rP, (idx - 1 >= lo) ? idx - 1 - E0 : -1, pv, pm, pmode);
            fresh = idx - 1 >= lo;
        }
    }
    __device__ __forceinline__ double value(int i, double dt) const { return lerp_nc(sv[i], dt, av[i]); }
};

// ---------------------------------------------------------------------------------------------------------
// Backward pass, consumer / helper wave pair per trajectory (2 x batch <= #SIMDs: a SIMD each).  The consumer wave runs the
// Riccati chain proper (backward_fused_body<.., PC = true>).  The helper wave evaluates what does not depend on the gains: this
// step's A, B columns (a4) and the cost tiles Lzz = Rz'WRz, [l_uu | l_u] = Ru'W[Ru | r] (a6), one step AHEAD of the consumer and
// handed over through a two-slot LDS ring, and the side products -- at the top of step t Tz = V Fz, Quz, Qzz (operands kept in
// registers since they were published), and, between the mid-step barrier and the end of the step (while the consumer forms the
// gains and V'), the tiles of step t-1.
// RU0 / RXC: r_u = 0 -- no r_u loads, no [l_uu | l_u] product, the ring's LU tiles stay zero; ONE constant r_x in
// registers (see backward_fused_body).
// SLP (differenced column store): per-DoF lists walked on the slope store (DownTrackerSlp).
template <int N, int M, bool RAWP = false, bool RU0 = false, bool RXC = false, bool SLP = false>
__device__ __forceinline__ void fusedpc_producer(double *pcbuf, int *sflag, RecLayout L, FusedArgs F, int T, const double *sh = nullptr, const int btraj = KP_BLOCK_TRAJ)
{
    static_assert(!SLP || !RAWP, "the slope store serves the helper on a differenced column store");
    static_assert(!RXC || RU0, "RXC comes with RU0");
    constexpr int n = N, m = M;
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int b = btraj;
    const int nr = F.nr, ncr = (nr + 3) >> 2;
    const int strideB = 3 * L.n * 8;                               // bytes of one key-point entry of kpc: three columns
    typename std::conditional<RAWP, DownTrackerRaw, typename std::conditional<SLP, DownTrackerSlp, DownTracker<8>>::type>::type tr;       // A rows then B rows of column c
    int oRx[4], oR1[4], oRu[4];
    d4 Wt, Wr;
    {
        double wt[4], wr[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 4 * r + q;
            tr.offs[r] = (row < n && c < n) ? 8 * ((c < F.dof ? 0 : n) + row) : BIGOFF;
            tr.offs[4 + r] = (row < n && c < m) ? 8 * (2 * n + row) : BIGOFF;
            oRx[r] = (row < nr && c < n) ? 8 * (row * n + c) : KP_OOB;
            oR1[r] = (row < nr && (c == n || RXC)) ? 8 * row : KP_OOB;      // (RXC: r[k] in every column, see CXX in backward_fused_body)
            oRu[r] = (row < nr && c < m) ? 8 * (row * m + c) : KP_OOB;
            wr[r] = (row < nr) ? 2.0 * F.w_run[row] : 0.0;
            wt[r] = (row < nr) ? 2.0 * F.w_term[row] : 0.0;
        }
        Wt.x = wt[0]; Wt.y = wt[1]; Wt.z = wt[2]; Wt.w = wt[3];
        Wr.x = wr[0]; Wr.y = wr[1]; Wr.z = wr[2]; Wr.w = wr[3];
    }
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    const int E0 = F.kp_offsets[(size_t)b * F.dof], NE = F.kp_offsets[(size_t)(b + 1) * F.dof] - E0;      // this trajectory's key-point entries
    __amdgpu_buffer_rsrc_t rT = kp_rsrc(F.kpc + (size_t)E0 * 3 * L.n, NE * strideB);
    const double *rb = F.r + (size_t)b * (T + 1) * nr;
    const double *rxb = F.r_x + (size_t)b * (T + 1) * nr * n;
    const double *rub = F.r_u + (size_t)b * (T + 1) * nr * m;
    d4 Rx, R1, Ru;
    // (the steps are asked for in order, T-1 first -- running pointers, as in backward_fused_body; with the 64-bit
    // (step x size) products the compiler formed the descriptors on the VALU and wrapped every load in a waterfall loop)
    const double *pRx = rxb + (size_t)(T - 1) * nr * n, *pR1 = rb + (size_t)(T - 1) * nr, *pRu = rub + (size_t)(T - 1) * nr * m;
    (void)pRx; (void)pR1; (void)pRu;
    auto load_res = [&](int t) {
        const bool ok = t >= 0;
        __amdgpu_buffer_rsrc_t rA = kp_rsrc(pRx, ok ? nr * n * 8 : 0);
        __amdgpu_buffer_rsrc_t rR = kp_rsrc(pR1, ok ? nr * 8 : 0);
        __amdgpu_buffer_rsrc_t rU = kp_rsrc(pRu, ok ? nr * m * 8 : 0);
        if (t > 0) { pRx -= nr * n; pR1 -= nr; pRu -= nr * m; }
        if constexpr (!RXC) { Rx.x = kp_bld(rA, oRx[0]); Rx.y = kp_bld(rA, oRx[1]); Rx.z = kp_bld(rA, oRx[2]); Rx.w = kp_bld(rA, oRx[3]); }
        R1.x = kp_bld(rR, oR1[0]); R1.y = kp_bld(rR, oR1[1]); R1.z = kp_bld(rR, oR1[2]); R1.w = kp_bld(rR, oR1[3]);
        if constexpr (!RU0) { Ru.x = kp_bld(rU, oRu[0]); Ru.y = kp_bld(rU, oRu[1]); Ru.z = kp_bld(rU, oRu[2]); Ru.w = kp_bld(rU, oRu[3]); }
    };
    // CXX: the constant block r_x' W r_x as a resident tile, Lzz~ = Cxx + 2 e_n (r_x' W r)' by ONE product (backward_fused_body)
    constexpr bool CXX = RXC;
    d4 Cxx = zero, RxW = zero;
    const double en2 = (c == n) ? 2.0 : 0.0;
    const u64 mask_r1 = (c == n) ? ~0ull : 0ull;
    (void)Cxx; (void)RxW; (void)en2; (void)mask_r1;
    if constexpr (RXC) {                           // the one r_x of the task: in registers for the whole sweep
        __amdgpu_buffer_rsrc_t rA = kp_rsrc(F.rx_const, nr * n * 8);
        Rx.x = kp_bld(rA, oRx[0]); Rx.y = kp_bld(rA, oRx[1]); Rx.z = kp_bld(rA, oRx[2]); Rx.w = kp_bld(rA, oRx[3]);
        if constexpr (CXX) { RxW = Rx * Wr; Cxx = kp_Pn(Rx, RxW, zero, ncr); }
    }
    if constexpr (RU0) {                           // [l_uu | l_u] = 0: both ring slots once (the consumer does not read them either)
        Ru = zero;
        kp_lds_store(pcbuf + 768, lane, zero); kp_lds_store(pcbuf + FPC_BUF + 768, lane, zero);
    }
    const int kd = (c < F.dof) ? c : c - F.dof;
    __amdgpu_buffer_rsrc_t rP = rT;
    if constexpr (RAWP) {
        rP = kp_rsrc(F.fdk + (size_t)E0 * (6 * n + 2) * 8, NE * (6 * n + 2) * 8);
        tr.init(rT, rP, F.kp_offsets, F.kp_times, c < n, (size_t)b * F.dof + kd, E0, NE, n, c < F.dof, F.eps2, F.rinv_2eps);
    } else if constexpr (SLP) {
        rP = kp_rsrc(F.kps + (size_t)E0 * 6 * L.n, NE * 2 * strideB);              // the trajectory's slice of the slope store
        tr.init(rP, F.kp_offsets, F.kp_times, c < n, (size_t)b * F.dof + kd, E0, NE, 2 * strideB);
    } else {
        tr.init(rT, F.kp_offsets, F.kp_times, c < n, (size_t)b * F.dof + kd, E0, NE, strideB);
    }
    (void)rP;
#pragma unroll
    for (int r = 0; r < 4; r++) if (c == n && 4 * r + q == n) tr.sv[r] = 1.0;       // Fz(n,n) = 1
    d4 hFz = zero, hFu = zero, hLzz = zero, hLU = zero;            // the tiles published last, for the side products of their step
    auto publish = [&](int t, const d4 &W2, auto terminal) __attribute__((always_inline)) {
        const double dt = (double)(t - tr.s);
        d4 Fz, Fu, Rz, Rur, Lzz;
        Fz.x = tr.value(0, dt); Fz.y = tr.value(1, dt); Fz.z = tr.value(2, dt); Fz.w = tr.value(3, dt);
        Fu.x = tr.value(4, dt); Fu.y = tr.value(5, dt); Fu.z = tr.value(6, dt); Fu.w = tr.value(7, dt);
        if constexpr (CXX && !decltype(terminal)::value) {
            double p = RxW.x * R1.x;
            p = __builtin_fma(RxW.y, R1.y, p); p = __builtin_fma(RxW.z, R1.z, p); p = __builtin_fma(RxW.w, R1.w, p);
            Lzz = KP_MFMA(en2, p, Cxx);
        } else {
            if constexpr (CXX) {
                Rz.x = bits_or(Rx.x, bits_and(R1.x, mask_r1)); Rz.y = bits_or(Rx.y, bits_and(R1.y, mask_r1));
                Rz.z = bits_or(Rx.z, bits_and(R1.z, mask_r1)); Rz.w = bits_or(Rx.w, bits_and(R1.w, mask_r1));
            } else {
                Rz.x = bits_or(Rx.x, R1.x); Rz.y = bits_or(Rx.y, R1.y); Rz.z = bits_or(Rx.z, R1.z); Rz.w = bits_or(Rx.w, R1.w);
            }
            Lzz = kp_Pn(Rz, Rz * W2, zero, ncr);
        }
        d4 LU = zero;
        if constexpr (!RU0) {
            Rur.x = bits_or(Ru.x, R1.x); Rur.y = bits_or(Ru.y, R1.y); Rur.z = bits_or(Ru.z, R1.z); Rur.w = bits_or(Ru.w, R1.w);
            LU = kp_Pn(Ru, Rur * W2, zero, ncr);
        }
        load_res(t - 1);
        double *tb = pcbuf + (t & 1) * FPC_BUF;
        // (Fz is the side products' operand only: it stays in this wave's registers)
        kp_lds_store(tb + 256, lane, Fu);
        // (Lzz: the consumer of the pair reads it at the terminal step only, V = Lzz(T-1); the side products take it
        // from registers here)
        if (t == T - 1) kp_lds_store(tb + 512, lane, Lzz);
        if constexpr (!RU0) kp_lds_store(tb + 768, lane, LU);
        hFz = Fz; hFu = Fu; hLzz = Lzz; hLU = LU;
    };
    load_res(T - 1);
    if (lane == 0) sflag[0] = 0;
    publish(T - 1, Wt, std::true_type{});                 // terminal weights   (iLQR.cpp:537-539)
    __syncthreads();
    constexpr int NCZ = (N + 1 + 3) / 4;
    constexpr int REG_NN = n >> 2;
    const bool lane_nn = (c == n) && (q == (n & 3));
    const u64 mask_n = (c == n) ? ~0ull : 0ull;
    // everything of step t that hangs on V but not on the gains, from the tiles this wave published for it
    auto side = [&](int t) __attribute__((always_inline)) {
        d4 V = hLzz;                                   // V_xx = l_xx[T-1]   (iLQR.cpp:537-539)
        if (t < T - 1) {                               // (V' + V'')/2 from the consumer's unsymmetrised image, as the consumer forms it
            V.x = 0.5 * (sh[KP_LDS_V + (q) * KP_VS + c] + sh[KP_LDS_V + c * KP_VS + q]);
            V.y = 0.5 * (sh[KP_LDS_V + (4 + q) * KP_VS + c] + sh[KP_LDS_V + c * KP_VS + 4 + q]);
            V.z = 0.5 * (sh[KP_LDS_V + (8 + q) * KP_VS + c] + sh[KP_LDS_V + c * KP_VS + 8 + q]);
            V.w = 0.5 * (sh[KP_LDS_V + (12 + q) * KP_VS + c] + sh[KP_LDS_V + c * KP_VS + 12 + q]);
            if (lane_nn) kp_set_reg<REG_NN>(V, 0.0);
        }
        d4 Luz;
        Luz.x = bits_and(hLU.x, mask_n); Luz.y = bits_and(hLU.y, mask_n); Luz.z = bits_and(hLU.z, mask_n); Luz.w = bits_and(hLU.w, mask_n);
        const d4 Tz = kp_P<NCZ>(V, hFz, zero);
        const d4 Quz = kp_P<NCZ>(hFu, Tz, Luz);
        const d4 Qzz = kp_P<NCZ>(hFz, Tz, hLzz);
        kp_lds_store(pcbuf + FPC_SIDE_QUZ, lane, Quz);
        kp_lds_store(pcbuf + FPC_SIDE_QZZ, lane, Qzz);
    };
    for (int t = T - 1; t > 0; t--) {
        side(t);
        __syncthreads();                               // mid-step: the consumer takes Quz, Qzz
        // the tiles of step t-1, while the consumer forms the gains and V' of step t (slot (t-1)&1 was last read at the top of step t+1)
        // (the crossing's arithmetic in front of the wait for the residual tiles, its requests behind it)
        // (the prefetched x+ / x- are differenced BEHIND the publish, whose wait for the residual tiles has let them arrive)
        if constexpr (RAWP) tr.cross(rT, t - 1, F.eps2, F.rinv_2eps);
        else tr.cross(t - 1);
        publish(t - 1, Wr, std::false_type{});
        if constexpr (RAWP) { tr.settle(rT, F.eps2, F.rinv_2eps); tr.request(rP, F.kp_times); }
        else if constexpr (SLP) tr.request(rP, F.kp_times, 2 * strideB);
        else tr.request(rT, F.kp_times, strideB);
        __syncthreads();                               // end of step: V of step t-1 is there
        if (__builtin_amdgcn_readfirstlane(sflag[0])) return;     // (wave-uniform: a divergent exit makes t a per-lane value and every request a waterfall loop)
    }
    side(0);
    __syncthreads();
    __syncthreads();
}

#define FPC_RING FLDS_TOTAL
#define FPC_FLAG (FPC_RING + 2 * FPC_BUF + 2 * 256)
#define FPC_TOTAL (FPC_FLAG + 2)
// guard: -1 run, 1 run only when the device flag says the key-point set is uniform, 0 only when it is not (the raw helper is
// launched for uniform sets; per-DoF lists go through k_fd_kp_difference and the plain / slope-store helper, launched behind it)
// Consumer / helper pair (2 x batch <= #SIMDs: a SIMD each, so always exclusive: no EXCL flag).  GATED (see k_backward_fused): consumer
// and helper of a settled trajectory, or of one that gave up, leave together, before the role split and before either touches the
// ring or its flags -- nobody is left waiting for a partner.  In a listed subset the role placement stays on the block index.
template <int N, int M, bool RAWP, bool RU0, bool RXC, bool SLP, bool GATED>
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_backward_fusedph(RecLayout L, FusedArgs F, int T, int role_shift, const double *__restrict__ lambda,
                   int pd_stride, double *__restrict__ Kout, double *__restrict__ kout,
                   double *__restrict__ delta_J, int *__restrict__ status, const int *__restrict__ kp_uniform, int guard,
                   const int *__restrict__ gate, const int *__restrict__ list)
{
    __shared__ __attribute__((aligned(16))) double sh[FPC_TOTAL];
    const int b = GATED ? kp_block_traj(list, KP_BLOCK_TRAJ) : KP_BLOCK_TRAJ;
    if constexpr (GATED) { if (gate[b] == 0) return; }
    if (guard >= 0 && (*kp_uniform != 0) != (guard != 0)) return;
    const bool consumer = ((__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) ^ (blockIdx.x >> role_shift)) & 1) == 0;
    if (consumer)
        backward_fused_body<N, M, true, RU0>(sh, sh + FPC_RING, (int *)(sh + FPC_FLAG), L, F, T, lambda, pd_stride, Kout, kout,
                                                   delta_J, status, nullptr, b);
    else
        fusedpc_producer<N, M, RAWP, RU0, RXC, SLP>(sh + FPC_RING, (int *)(sh + FPC_FLAG), L, F, T, sh, b);
}
// ---------------------------------------------------------------------------------------------------------
// Forward pass.  The column tracker walks UP in time; its tiles (row = A row, col = A column) are turned into
// the Y operands (row = contraction index) through a padded LDS transpose, off the Z dependency chain.
// The time loop of the forward sweep by register set: NS consecutive steps with compile-time set indices, and what is left
// below a full group at the end (MODE 1 ends in the final step, mode 3, at t = T-1; MODE 0 has no final step of its own).
// The role tag of a step (paired scoring, see PAIR2 in forward_fused_body): 0 the step scores itself with its own r_x product
// (every form but the paired one), 1 the even member of a pair (no scoring: its Z stays live), 2 the odd member (ONE product
// scores both), 3 a step of the paired form that scores itself (the step in front of the final one when it has no partner, and
// the final step).  P2: the sets pair up as (0, 1), (2, 3).
template <int K, int NS, int MODE, bool P2 = false, class StepF>
__device__ __forceinline__ void fwd_steps(StepF &step, int t)
{
    step(t, std::integral_constant<int, MODE>{}, std::integral_constant<int, K>{}, std::integral_constant<int, P2 ? 1 + (K & 1) : 0>{});
    if constexpr (K + 1 < NS) fwd_steps<K + 1, NS, MODE, P2>(step, t + 1);
}
template <int K, int NS, int MODE, class StepF>
__device__ __forceinline__ void fwd_tail(StepF &step, int t, int T)
{
    if constexpr (MODE == 0) {
        if (t < T) {
            step(t, std::integral_constant<int, 0>{}, std::integral_constant<int, K>{}, std::integral_constant<int, 0>{});
            if constexpr (K + 1 < NS) fwd_tail<K + 1, NS, 0>(step, t + 1, T);
        }
    } else {
        if (K + 1 == NS || t == T - 1) step(T - 1, std::integral_constant<int, 3>{}, std::integral_constant<int, K>{}, std::integral_constant<int, 0>{});
        else {
            step(t, std::integral_constant<int, MODE>{}, std::integral_constant<int, K>{}, std::integral_constant<int, 0>{});
            if constexpr (K + 1 < NS) fwd_tail<K + 1, NS, MODE>(step, t + 1, T);
        }
    }
}

// RXC: one r_x [nr][n] for every trajectory and step (see backward_fused_body): its transposed tile stays in registers, the
// sweep issues no r_x loads (4 of a step's 15) and the four tile sets shrink by a tile each.
// PAIR2 (with RXC, RU0, UNI; n_alpha <= 8, FusedLaunch::pair2): ONE scoring product per two steps, see P2 below.
template <int NCZ, int NCU, bool RU0 = false, bool UNI = false, bool RXC = false, bool PAIR2 = false>
__device__ __forceinline__ void forward_fused_body(RecLayout L, FusedArgs F, int T, int n_alpha, const double *__restrict__ Kin, const double *__restrict__ kin,
               const double *__restrict__ u_nom, const double *__restrict__ ctrl_lim,
               const double *__restrict__ alphas, double *__restrict__ cost_pred, double *__restrict__ U_alpha, const int btraj = KP_BLOCK_TRAJ)
{
    __shared__ __attribute__((aligned(16))) double shA[16 * 17], shB[16 * 17];
    // The chunk counts name the shape (KP_T1_SHAPES: (14,7) -> <4,2>, (4,1) -> <2,1>, (12,3) -> <4,1>, (10,3) -> <3,1>; the
    // launcher dispatches nothing else), so n and m are compile-time constants here as in the backward sweep: the row of k in
    // the gain operand, the chunk count of r_x dx and the row masks cost no selects or scalar branches per step.
    constexpr int n = (NCZ == 4 && NCU == 2) ? 14 : (NCZ == 2) ? 4 : (NCZ == 4) ? 12 : 10;
    constexpr int m = (NCZ == 4 && NCU == 2) ? 7 : (NCZ == 2) ? 1 : 3;
    const int lane = threadIdx.x, c = lane & 15, q = lane >> 4;
    const int b = btraj;
    const int nr = F.nr;
    constexpr int strideB = 3 * n * 8;                             // bytes of one key-point entry of kpc: three columns
    constexpr int ncx = (n + 3) >> 2;

    // this trajectory's key-point entries [E0, E0 + NE) of kpc; KpU: entries per DoF list when all lists are the same (UNI)
    const int E0 = F.kp_offsets[(size_t)b * F.dof], NE = F.kp_offsets[(size_t)(b + 1) * F.dof] - E0;
    const int KpU = F.kp_offsets[(size_t)b * F.dof + 1] - E0;
    ColOffs co;
    if (!UNI) col_offsets(co, n, m, F.dof, c, q);
    int oK[4], oRxT[4], oRuT[4], oR[4], oub[4];
    double lo[NCU], hi[NCU], wcur[4];
    // RV2 (uniform key-point sets): the residuals sit in the rows of Jx, Ju in the order
    //     row 4r + q  <->  residual sig(4r + q) = 8 (r >> 1) + 2 q + (r & 1)
    // so that registers (0, 1) and (2, 3) of a lane are CONSECUTIVE residuals and r_t arrives with two 16-byte requests instead of four
    // 8-byte ones (a request costs this sweep ~24 cycles of its 1 330-cycle step whatever it carries: timing probe in
    // profiles/r05_headline_ab.txt).  The order is a relabelling of the rows of the resident r_x tile and of the per-row constants.
    constexpr bool RV2 = UNI;        // (the per-DoF list form measured 1.3 % SLOWER with it: 2.31 against 2.28 ms)
    auto sig = [](int i) { return RV2 ? 8 * (i >> 3) + 2 * (i & 3) + ((i >> 2) & 1) : i; };
    const int cs = sig(c);                                                  // the residual in column c of the RxT operand
    const int oR2[2] = {(2 * q < nr) ? 16 * q : KP_OOB, (8 + 2 * q < nr) ? 64 + 16 * q : KP_OOB};
    (void)oR2;
    // P2 (paired scoring): the r_x product sits off the state chain, its first operand is the same resident tile at every step and
    // column c of its result depends on column c of Z alone -- and the candidates fill n_alpha <= 8 of the tile's 16 columns.  So the
    // running steps pair up by register set, (0, 1) and (2, 3): the even member (step t) issues no scoring product and keeps its Z;
    // the odd member (step t+1) moves columns 0..7 of Z_t into columns 8..15 of its own Z -- a masked row shift, two 32-bit moves
    // per register, behind the last product of the state chain that reads the tile, so the chain never sees them -- and ONE product
    // scores both: lanes c < 8 accumulate step t+1, lanes c >= 8 step t, folded behind the sweep.  r arrives once per pair, with the
    // same two 16-byte requests: lanes c < 8 read the row above (a per-lane byte offset of one row).  The over-read of an odd
    // residual count (see RV2 below) then reaches one element past row t+1: pairs end at step T-2, so it stays inside the T + 1 rows.
    // The final step (terminal weights, its own tile) and a step T-2 left without a partner score themselves as before.
    constexpr bool P2 = PAIR2 && RXC && RU0 && UNI;
    static_assert(!P2 || (KP_FWD_SETS & 1) == 0, "paired scoring pairs the register sets");
    const int oR2p[2] = {oR2[0] == KP_OOB ? KP_OOB : oR2[0] + (c < 8 ? nr * 8 : 0), oR2[1] == KP_OOB ? KP_OOB : oR2[1] + (c < 8 ? nr * 8 : 0)};
    (void)oR2p;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = 4 * r + q;
        if (UNI) {
            // the Y operands themselves: Ya(p = row, o = c) = A(o, p), Yb(p, o) = B(o, p) -- element c of column `row`, whose
            // DoF list starts (row mod dof) * KpU entries into the trajectory's slice (equal lists: the same position in each)
            const int d = row < F.dof ? row : row - F.dof;
            co.a[r] = (row < n && c < n) ? 8 * ((d * KpU * 3 + (row < F.dof ? 0 : 1)) * n + c) : BIGOFF;
            co.b[r] = (row < m && c < n) ? 8 * ((row * KpU * 3 + 2) * n + c) : BIGOFF;
        }
        oK[r] = (row < n && c < m) ? 8 * (row * m + c) : KP_OOB;
        oRxT[r] = (row < n && cs < nr) ? 8 * (cs * n + row) : KP_OOB;   // RxT(p=row, k=c) = r_x[k][p]   (RV2: residual sig(c) in column c)
        oRuT[r] = (row < m && cs < nr) ? 8 * (cs * m + row) : KP_OOB;   // RuT(p=row, k=c) = r_u[k][p]
        oR[r] = (row < nr) ? 8 * row : KP_OOB;                          // r[k=row] (rows of Jx / Ju; RV2: oR2)
        oub[r] = (row < m) ? 8 * row : KP_OOB;
        if (r < NCU) {
            lo[r] = (row < m) ? ctrl_lim[2 * row] : -1.0e300;
            hi[r] = (row < m) ? ctrl_lim[2 * row + 1] : 1.0e300;
        }
        wcur[r] = (sig(row) < nr) ? F.w_run[sig(row)] : 0.0;
    }
    constexpr int rn = n >> 2;                                              // the register of row n (k)
    const int okn = (q == (n & 3) && c < m) ? 8 * c : KP_OOB;
    const double my_alpha = (c < n_alpha) ? alphas[c] : 0.0;
    d4 Z;
    {
        double zr[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 4 * r + q;
            zr[r] = (row == n) ? my_alpha : (row == n + 1) ? 1.0 : 0.0;
        }
        Z.x = zr[0]; Z.y = zr[1]; Z.z = zr[2]; Z.w = zr[3];
    }
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    double partial = 0.0;

    __amdgpu_buffer_rsrc_t rT = kp_rsrc(F.kpc + (size_t)E0 * 3 * L.n, NE * strideB);
    const double *rb = F.r + (size_t)b * (T + 1) * nr;
    const double *rxb = F.r_x + (size_t)b * (T + 1) * nr * n;
    const double *rub = F.r_u + (size_t)b * (T + 1) * nr * m;

    struct Tiles { d4 YkK, RxT, RuT, rv, ub; double kk; };      // kk: this lane's element of k (row n of Yk lives in ONE register)
    auto load_tiles = [&](int t, Tiles &s) {
        __amdgpu_buffer_rsrc_t rK = kp_rsrc(Kin + ((size_t)b * T + t) * m * n, m * n * 8);
        __amdgpu_buffer_rsrc_t rk = kp_rsrc(kin + ((size_t)b * T + t) * m, m * 8);
        __amdgpu_buffer_rsrc_t ru = kp_rsrc(u_nom + ((size_t)b * T + t) * m, m * 8);
        __amdgpu_buffer_rsrc_t rRx = kp_rsrc(rxb + (size_t)t * nr * n, nr * n * 8);
        __amdgpu_buffer_rsrc_t rRu = kp_rsrc(rub + (size_t)t * nr * m, nr * m * 8);
        __amdgpu_buffer_rsrc_t rR = kp_rsrc(rb + (size_t)t * nr, nr * 8);
        s.YkK.x = kp_bld(rK, oK[0]); s.YkK.y = kp_bld(rK, oK[1]); s.YkK.z = kp_bld(rK, oK[2]); s.YkK.w = kp_bld(rK, oK[3]);
        s.kk = kp_bld(rk, okn);
        if constexpr (!RXC) { s.RxT.x = kp_bld(rRx, oRxT[0]); s.RxT.y = kp_bld(rRx, oRxT[1]); s.RxT.z = kp_bld(rRx, oRxT[2]); s.RxT.w = kp_bld(rRx, oRxT[3]); }
        if constexpr (!RU0) {
            s.RuT.x = kp_bld(rRu, oRuT[0]); s.RuT.y = NCU > 1 ? kp_bld(rRu, oRuT[1]) : 0.0;
            s.RuT.z = NCU > 2 ? kp_bld(rRu, oRuT[2]) : 0.0; s.RuT.w = NCU > 3 ? kp_bld(rRu, oRuT[3]) : 0.0;
        }
        if constexpr (P2) {             // (r belongs to the pair: requested behind the tiles, below)
        } else if constexpr (RV2) {
            // (descriptor one element longer: the last pair of an odd residual count reaches into the next step's row -- the array has
            // T + 1 rows, the weights beyond nr are zero)
            __amdgpu_buffer_rsrc_t rR2 = kp_rsrc(rb + (size_t)t * nr, nr * 8 + 8);
            double r0, r1, r2, r3;
            kp_bld2s(rR2, oR2[0], 0, r0, r1); kp_bld2s(rR2, oR2[1], 0, r2, r3);
            s.rv.x = r0; s.rv.y = r1; s.rv.z = r2; s.rv.w = r3;
        } else {
        s.rv.x = kp_bld(rR, oR[0]); s.rv.y = kp_bld(rR, oR[1]); s.rv.z = kp_bld(rR, oR[2]); s.rv.w = kp_bld(rR, oR[3]);
        }
        s.ub.x = kp_bld(ru, oub[0]); s.ub.y = NCU > 1 ? kp_bld(ru, oub[1]) : 0.0;
        s.ub.z = NCU > 2 ? kp_bld(ru, oub[2]) : 0.0; s.ub.w = NCU > 3 ? kp_bld(ru, oub[3]) : 0.0;
    };

    // ---- column tracker, walking UP in time --------------------------------------------------------------
    // UNI: every DoF of the trajectory has the SAME key-point list (set_interval, and whatever else comes out uniform), so
    // one list serves all four registers of a lane and the lanes interpolate the transposed operands Ya, Yb directly --
    // lane (q, c) holds A(c, 4r+q): row c of A, a different COLUMN (DoF list) per register otherwise, which is why the
    // general form interpolates column-wise and transposes through LDS
    const int kd = UNI ? 0 : (c < F.dof) ? c : c - F.dof;
    const bool has = c < n;
    const int klo = has ? F.kp_offsets[(size_t)b * F.dof + kd] : 0;
    const int khi = has ? F.kp_offsets[(size_t)b * F.dof + kd + 1] : 0;
    int idx = klo;
    int s = has ? F.kp_times[idx] : 0;                                  // == 0 for canonical key-points
    int e = (has && idx + 1 < khi) ? F.kp_times[idx + 1] : BIGT;
    int nb = (has && idx + 2 < khi) ? F.kp_times[idx + 2] : BIGT;
    // General form (!UNI): the slope store of k_kp_slopes gives every segment's slope with its start column -- requested one
    // crossing ahead (ev, ea), so a crossing is register moves and nothing is waited for at the step behind it.
    double sv[8], ev[8], av[8], ea[8];
    (void)ea;
    __amdgpu_buffer_rsrc_t rS = rT;
    load_col(rT, co, has ? idx - E0 : -1, NE, strideB, sv);
    load_col(rT, co, (has && idx + 1 < khi) ? idx + 1 - E0 : -1, NE, strideB, ev);
#pragma unroll
    for (int i = 0; i < 8; i++) av[i] = 0.0;
    if constexpr (!UNI) {
        rS = kp_rsrc(F.kps + (size_t)E0 * 6 * L.n, NE * 2 * strideB);
        load_col2(rS, co, has ? idx - E0 : -1, NE, 2 * strideB, sv, av);
        load_col2(rS, co, (has && idx + 1 < khi) ? idx + 1 - E0 : -1, NE, 2 * strideB, ev, ea);
    }
    // the identity rows of Ya (alpha and the homogeneous 1 carry over): lanes c >= n walk no list
#pragma unroll
    for (int r = 0; r < 4; r++) if ((c == n || c == n + 1) && 4 * r + q == c) sv[r] = 1.0;

    // Two register sets: S0 holds the tiles of the even steps, S1 those of the odd ones; step t re-requests ITS set for step
    // t+2 right behind each tile's last use.  A wavefront's loads return in order and a step is shorter than a trip to HBM
    // (the sweep ran at one memory latency per step with a single set: 2.66 ms at B = 128 where its arithmetic needs 2.13,
    // -DKP_PROBE_SAMEB), so the requests have to be two steps ahead of their use.
    // (the general form with control residuals keeps four sets: with six its largest shape spills -- 100 bytes of scratch, tools/isa_lint.py)
    constexpr int NS = UNI ? KP_FWD_SETS : (RU0 || KP_FWD_SETS_GEN < 4) ? KP_FWD_SETS_GEN : 4;
    Tiles S[NS];
    d4 RxTc = {0.0, 0.0, 0.0, 0.0}, RxTt = RxTc;
    // SQW (round 5; constant r_x, no control residuals, uniform key-point sets -- the headline's forward sweep): the ROWS of the
    // resident r_x are scaled by sqrt(w_k) once (a second tile carries the terminal weights), so the product gives Js = sqrt(w) Jx and
    //     sum_k w_k Jx_k (2 r_k + Jx_k)  =  sum_k Js_k (2 sqrt(w_k) r_k + Js_k)
    // is two FMAs per register instead of an add, a multiply, an FMA and the doubling of r: 8 VALU instructions less of the step's
    // 79 (a lone wave pays for each).  sqrt(w) is correctly rounded; the costs move by ~1e-16 relative (held to the oracle at 1e-9).
    // A NEGATIVE weight (legal: the reference just forms w r^2) keeps its sign outside the root: the rows are scaled by sqrt|w_k|, every
    // register accumulates its own residual's terms (acc4: register r of lane (c, q) is residual 4r + q throughout), and the signs
    // join once, behind the sweep (the final step, whose terminal weights have signs of their own, is added with them directly).
    constexpr bool SQW = RXC && RU0 && UNI;
    double s2run[4] = {0.0, 0.0, 0.0, 0.0}, s2term[4] = {0.0, 0.0, 0.0, 0.0}, sgrun[4] = {1.0, 1.0, 1.0, 1.0}, sgterm[4] = {1.0, 1.0, 1.0, 1.0};
    double acc4[4] = {0.0, 0.0, 0.0, 0.0};
    (void)s2run; (void)s2term; (void)RxTt; (void)sgrun; (void)sgterm; (void)acc4;
    if constexpr (RXC) {
        __amdgpu_buffer_rsrc_t rRxc = kp_rsrc(F.rx_const, nr * n * 8);
        RxTc.x = kp_bld(rRxc, oRxT[0]); RxTc.y = kp_bld(rRxc, oRxT[1]); RxTc.z = kp_bld(rRxc, oRxT[2]); RxTc.w = kp_bld(rRxc, oRxT[3]);
        if constexpr (SQW) {
            // lane (c, q) of the operand tile holds r_x[k = c][p = 4r + q]: column c is residual c
            const double swr = (cs < nr) ? __builtin_sqrt(fabs(F.w_run[cs])) : 0.0, swt = (cs < nr) ? __builtin_sqrt(fabs(F.w_term[cs])) : 0.0;
            RxTt = RxTc * swt;
            RxTc = RxTc * swr;
#pragma unroll
            for (int r = 0; r < 4; r++) {           // the scoring side: residual k = 4r + q in register r
                const int kr = sig(4 * r + q);
                const double wr_ = (kr < nr) ? F.w_run[kr] : 0.0, wt_ = (kr < nr) ? F.w_term[kr] : 0.0;
                s2run[r] = 2.0 * __builtin_sqrt(fabs(wr_)); sgrun[r] = wr_ < 0.0 ? -1.0 : 1.0;
                s2term[r] = 2.0 * __builtin_sqrt(fabs(wt_)); sgterm[r] = wt_ < 0.0 ? -1.0 : 1.0;
            }
        }
    }
    (void)RxTc;
#pragma unroll
    for (int k = 0; k < NS; k++) load_tiles(k < T ? k : T - 1, S[k]);
    if constexpr (P2) {
        // r of the pairs (k, k + 1), kept in the even set: rows k and k + 1 of the T + 1, one element more for the over-read of an
        // odd residual count; a pair that does not exist at this horizon fetches the last one that could (never used)
#pragma unroll
        for (int k = 0; k < NS; k += 2) {
            const int tk = k + 2 < T ? k : (T > 2 ? T - 2 : 0), rows = T + 1 - tk;
            __amdgpu_buffer_rsrc_t rRp = kp_rsrc(rb + (size_t)tk * nr, rows > 2 ? 2 * nr * 8 + 8 : rows * nr * 8);
            double r0, r1, r2, r3;
            kp_bld2s(rRp, oR2p[0], 0, r0, r1); kp_bld2s(rRp, oR2p[1], 0, r2, r3);
            S[k].rv.x = r0; S[k].rv.y = r1; S[k].rv.z = r2; S[k].rv.w = r3;
        }
    }

    // One wavefront per workgroup: LDS accesses of the wave execute in order, so the write -> transposed read
    // pairs below need no barrier.  The Y operands of step t+1 are produced during step t (off the Z chain).
    auto stage_cols = [&](int t) {            // a4 in the column layout -> LDS
        const double dt = (double)(t - s);
        shA[(q) * 17 + c] = lerp_nc(sv[0], dt, av[0]);      shA[(4 + q) * 17 + c] = lerp_nc(sv[1], dt, av[1]);
        shA[(8 + q) * 17 + c] = lerp_nc(sv[2], dt, av[2]);  shA[(12 + q) * 17 + c] = lerp_nc(sv[3], dt, av[3]);
        shB[(q) * 17 + c] = lerp_nc(sv[4], dt, av[4]);      shB[(4 + q) * 17 + c] = lerp_nc(sv[5], dt, av[5]);
        shB[(8 + q) * 17 + c] = lerp_nc(sv[6], dt, av[6]);  shB[(12 + q) * 17 + c] = lerp_nc(sv[7], dt, av[7]);
    };
    auto fetch_Y = [&](d4 &Ya, d4 &Yb) {      // Ya(p, o) = A(o, p);  Yb(p, o) = B(o, p)
        Ya.x = shA[c * 17 + q];      Ya.y = shA[c * 17 + 4 + q];
        Ya.z = shA[c * 17 + 8 + q];  Ya.w = shA[c * 17 + 12 + q];
        Yb.x = shB[c * 17 + q];                Yb.y = NCU > 1 ? shB[c * 17 + 4 + q] : 0.0;
        Yb.z = NCU > 2 ? shB[c * 17 + 8 + q] : 0.0; Yb.w = NCU > 3 ? shB[c * 17 + 12 + q] : 0.0;
    };
    auto advance = [&](int t) {             // the general form's per-lane tracker
        if constexpr (!UNI) {
            // A lane that reaches the end key-point of its segment takes the (value, slope) pairs requested a crossing ago -- register
            // moves -- and requests the pairs of the segment after.  The REQUESTS are issued by ALL lanes, behind a wave-uniform
            // branch ("some lane crosses"): a lane that does not cross re-requests the entry it already holds.  With the loads inside
            // the per-lane branch their results met the old values at the join of the branch -- copies of freshly loaded registers,
            // i.e. `s_waitcnt vmcnt(0)` on EVERY step: the wave drained its four tile sets in flight once per step and ran at one
            // trip to HBM per step (2.7 ms where the uniform form takes 1.8).  Now nothing waits for these loads before the
            // lane's next crossing.
            const bool cr = t >= e;
            if (__builtin_amdgcn_ballot_w64(cr) != 0) {
                if (cr) {
#pragma unroll
                    for (int i = 0; i < 8; i++) { sv[i] = ev[i]; av[i] = ea[i]; }
                    s = e; e = nb; idx++;
                }
                const int en = (idx + 1 < khi) ? idx + 1 - E0 : -1;
                load_col2(rS, co, en, NE, 2 * strideB, ev, ea);
                nb = (idx + 2 < khi) ? F.kp_times[idx + 2] : BIGT;
            }
        }
    };
    // Y operands: step t uses (Ya, Yb); during step t the tiles of step t+1 are fetched from LDS (staged during
    // step t-1) and those of step t+2 are staged.
    d4 Ya, Yb;
    auto lerp_Y = [&](int t) {                // UNI: the operands of step t straight from the tracker
        const double dt = (double)(t - s);
        Ya.x = lerp_nc(sv[0], dt, av[0]); Ya.y = lerp_nc(sv[1], dt, av[1]); Ya.z = lerp_nc(sv[2], dt, av[2]); Ya.w = lerp_nc(sv[3], dt, av[3]);
        Yb.x = lerp_nc(sv[4], dt, av[4]); Yb.y = NCU > 1 ? lerp_nc(sv[5], dt, av[5]) : 0.0;
        Yb.z = NCU > 2 ? lerp_nc(sv[6], dt, av[6]) : 0.0; Yb.w = NCU > 3 ? lerp_nc(sv[7], dt, av[7]) : 0.0;
    };
    if (UNI) lerp_Y(0);
    else {
        stage_cols(0);
        fetch_Y(Ya, Yb);
        if (T > 1) { advance(1); stage_cols(1); }
    }

    // one descriptor per array for the whole trajectory; the step (t+1, or t again behind the last one: never used) goes
    // into the loads' scalar offset
    const __amdgpu_buffer_rsrc_t rK = kp_rsrc(Kin + (size_t)b * T * m * n, T * m * n * 8), rk = kp_rsrc(kin + (size_t)b * T * m, T * m * 8),
                                 ru = kp_rsrc(u_nom + (size_t)b * T * m, T * m * 8), rRx = kp_rsrc(rxb, (T + 1) * nr * n * 8),
                                 rRu = kp_rsrc(rub, (T + 1) * nr * m * 8), rR = kp_rsrc(rb, (T + 1) * nr * 8);
    // UNI: the uniform tracker of the segment loop below (positions and times are wave-uniform scalars)
    int up = 0, uks = 0, uke = 0, ukn_v = 0;            // segment's start position, its start / end time, the time after that (as loaded)
    double ev2[8];                                       // the column after the next one (requested a segment ahead)
    double wterm[4] = {0.0, 0.0, 0.0, 0.0};
    (void)up; (void)uks; (void)uke; (void)ukn_v; (void)ev2; (void)wterm;
    // MODE 0: the general form (per-lane tracker, crossing inside the step); UNI: 1 a step below T-1 -- when it is the last one
    // of its segment, the crossing into the next segment sits behind a wave-uniform scalar branch where the general form advances
    // its per-lane tracker; 3 the final step t = T-1 (terminal weights, nothing left to request).
    // The tile requests stay OUTSIDE every branch and the loop has one body (a pair of steps): a request in flight across a
    // join of paths that each issued it ends in register copies at the join, and a copy waits for the load (a form with the
    // crossing step peeled into straight-line code had `s_waitcnt vmcnt(0)` plus 16 moves at the end of every segment).
    // PAR: the parity of t (which register set the step works on)
    d4 Zev = zero, rvE = zero, rvF = zero;          // P2: Z of a pair's even member; r of the two steps that score themselves (T-2, T-1)
    (void)Zev; (void)rvE; (void)rvF;
    auto step = [&](int t, auto mode_tag, auto par_tag, auto role_tag) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode_tag)::value;
        constexpr int PAR = decltype(par_tag)::value;
        constexpr int ROLE = P2 ? decltype(role_tag)::value : 0;      // (see fwd_steps)
        static_assert(!P2 || (ROLE >= 1 && ROLE <= 3 && (MODE != 3 || ROLE == 3)), "a step of the paired form has a role");
        Tiles &cur = S[PAR];
        const bool more = MODE == 3 ? false : MODE != 0 ? true : t + 1 < T;
        const int tn = MODE == 3 ? t : (t + NS < T ? t + NS : T - 1);       // (behind the last steps: a valid address, never used)
        const int sK = tn * m * n * 8, sk = tn * m * 8, sRx = tn * nr * n * 8, sRu = tn * nr * m * 8, sR = tn * nr * 8;
        (void)sRu;
        // Order of the step: every product is a dependent MFMA chain whose result is usable ~100 cycles after its last
        // issue, so independent work is placed behind each chain before its consumer:
        //   U chain | A dx chain | clamp (U ready) | B du | r_u du | r_x dx | a4 of step t+1 (VALU + LDS) | cost (Jx ready)
        d4 Yk = cur.YkK;                               // + k in row n (the lanes of the other rows hold 0): ONE load, not a tile of four
        if constexpr (rn == 3) Yk.w += cur.kk; else if constexpr (rn == 2) Yk.z += cur.kk; else if constexpr (rn == 1) Yk.y += cur.kk; else Yk.x += cur.kk;
        const d4 ub = cur.ub;
        // TRIM (round 5, the uniform form): the product starts from zero and u_nom joins on the VALU in the registers that hold
        // controls -- as the accumulator's initial value the tile had to be assembled first: seven moves per step -- and the clamp is
        // v_min / v_max: 1.74 -> 1.68 ms.  (The general form measured 3 % SLOWER with the same change and keeps the old code.)
        constexpr bool TRIM = UNI;
        d4 U = kp_P<NCZ>(Yk, Z, TRIM ? zero : ub);       // (u_nom +) K dx + alpha k   (:879)
        __builtin_amdgcn_sched_barrier(0);
        cur.YkK.x = kp_blds(rK, oK[0], sK); cur.YkK.y = kp_blds(rK, oK[1], sK); cur.YkK.z = kp_blds(rK, oK[2], sK); cur.YkK.w = kp_blds(rK, oK[3], sK);
        cur.kk = kp_blds(rk, okn, sk);
        __builtin_amdgcn_sched_barrier(0);
        d4 Zn = kp_P<NCZ>(Ya, Z, zero);                  // A dx (does not need the controls)
        __builtin_amdgcn_sched_barrier(0);
        d4 dU;
        {
            double u;
            // rows >= 4*NCU of U hold no control (exact zeros): only the first NCU registers are clamped (:883-889)
            dU = zero;
            if constexpr (TRIM) {
            u = vmax64(vmin64(U.x + ub.x, hi[0]), lo[0]); U.x = u; dU.x = u - ub.x;
            if constexpr (NCU > 1) { u = vmax64(vmin64(U.y + ub.y, hi[1]), lo[1]); U.y = u; dU.y = u - ub.y; }
            if constexpr (NCU > 2) { u = vmax64(vmin64(U.z + ub.z, hi[2]), lo[2]); U.z = u; dU.z = u - ub.z; }
            if constexpr (NCU > 3) { u = vmax64(vmin64(U.w + ub.w, hi[3]), lo[3]); U.w = u; dU.w = u - ub.w; }
            } else {
            u = U.x; if (u > hi[0]) u = hi[0]; if (u < lo[0]) u = lo[0]; U.x = u; dU.x = u - ub.x;
            if constexpr (NCU > 1) { u = U.y; if (u > hi[1]) u = hi[1]; if (u < lo[1]) u = lo[1]; U.y = u; dU.y = u - ub.y; }
            if constexpr (NCU > 2) { u = U.z; if (u > hi[2]) u = hi[2]; if (u < lo[2]) u = lo[2]; U.z = u; dU.z = u - ub.z; }
            if constexpr (NCU > 3) { u = U.w; if (u > hi[3]) u = hi[3]; if (u < lo[3]) u = lo[3]; U.w = u; dU.w = u - ub.w; }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        cur.ub.x = kp_blds(ru, oub[0], sk); cur.ub.y = NCU > 1 ? kp_blds(ru, oub[1], sk) : 0.0;
        cur.ub.z = NCU > 2 ? kp_blds(ru, oub[2], sk) : 0.0; cur.ub.w = NCU > 3 ? kp_blds(ru, oub[3], sk) : 0.0;
        __builtin_amdgcn_sched_barrier(0);
        Zn = kp_P<NCU>(Yb, dU, Zn);                      // + B du: the next state
        d4 Ju = zero;                                  // RU0: r_u = 0, the control residual term vanishes
        if constexpr (!RU0) Ju = kp_P<NCU>(cur.RuT, dU, zero);
        d4 Jx = zero;
        if constexpr (ROLE == 1) Zev = Z;                  // scored by the odd member
        else {
            if constexpr (ROLE == 2) {
                // columns 8..15 of Z <- columns 0..7 of the even member's Z (row_shr:8 under bank mask 0xc: lanes 8..15 of every row of
                // 16 take the value 8 lanes below, lanes 0..7 keep theirs).  Every product of the state chain that reads Z has been
                // issued above; Z is replaced right below, so the chain never carries these columns.
                auto put = [](double dst, double src) {
                    const u32x2 d = __builtin_bit_cast(u32x2, dst), s = __builtin_bit_cast(u32x2, src);
                    const u32x2 o = {(unsigned)__builtin_amdgcn_update_dpp((int)d.x, (int)s.x, 0x118, 0xf, 0xc, false),
                                      (unsigned)__builtin_amdgcn_update_dpp((int)d.y, (int)s.y, 0x118, 0xf, 0xc, false)};
                    return __builtin_bit_cast(double, o);
                };
                Z.x = put(Z.x, Zev.x);
                if constexpr (ncx > 1) Z.y = put(Z.y, Zev.y);
                if constexpr (ncx > 2) Z.z = put(Z.z, Zev.z);
                if constexpr (ncx > 3) Z.w = put(Z.w, Zev.w);
            }
            Jx = kp_P<ncx>(RXC ? ((SQW && MODE == 3) ? RxTt : RxTc) : cur.RxT, Z, zero);     // (SQW: sqrt(w) Jx; terminal weights at the final step)
        }
        Z = Zn;
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!RXC) { cur.RxT.x = kp_blds(rRx, oRxT[0], sRx); cur.RxT.y = kp_blds(rRx, oRxT[1], sRx); cur.RxT.z = kp_blds(rRx, oRxT[2], sRx); cur.RxT.w = kp_blds(rRx, oRxT[3], sRx); }
        if constexpr (!RU0) {
            cur.RuT.x = kp_blds(rRu, oRuT[0], sRu); cur.RuT.y = NCU > 1 ? kp_blds(rRu, oRuT[1], sRu) : 0.0;
            cur.RuT.z = NCU > 2 ? kp_blds(rRu, oRuT[2], sRu) : 0.0; cur.RuT.w = NCU > 3 ? kp_blds(rRu, oRuT[3], sRu) : 0.0;
        }
        if (!UNI && more) fetch_Y(Ya, Yb);             // Y operands of step t+1 (staged during step t-1 ... see below)
        __builtin_amdgcn_sched_barrier(0);
        if (U_alpha && c < n_alpha) {
            double *Ua = U_alpha + (((size_t)b * n_alpha + c) * T + t) * m;
            const double uv[4] = {U.x, U.y, U.z, U.w};
#pragma unroll
            for (int r = 0; r < NCU; r++) { const int row = 4 * r + q; if (row < m) Ua[row] = uv[r]; }
        }
        // a4 for step t+2 (column layout -> LDS): fills the latency of the products above
        if constexpr (MODE == 0) {
            if (UNI) { if (more) { advance(t + 1); lerp_Y(t + 1); } }
            else if (t + 2 < T) { advance(t + 2); stage_cols(t + 2); }
        } else if constexpr (MODE == 1) {
            if (t + 1 == uke) {
                // crossing into segment up + 1: its start column (ev) and end column (ev2) were requested one and two segments
                // ago; the column after those and its time are requested now, the time BEHIND the columns (loads return in
                // order: a wait that leaves "the youngest loads" in flight must not have to sit out the time's latency)
                const int kn = __builtin_amdgcn_readfirstlane(ukn_v);
                uks = uke; uke = kn; up++;
                const int gap = uke - uks;
                const double den = (double)(gap > 0 ? gap : 1), rinv = kp_rcp(den);
#pragma unroll
                for (int i = 0; i < 8; i++) { sv[i] = ev[i]; ev[i] = ev2[i]; av[i] = fdiv(ev[i] - sv[i], den, rinv); }
                if (c == n || c == n + 1) {                                // the identity rows of Ya: lanes c >= n walk no list
#pragma unroll
                    for (int r = 0; r < 4; r++) if (4 * r + q == c) { sv[r] = 1.0; ev[r] = 1.0; av[r] = 0.0; }
                }
                const int pn = up + 2 < KpU ? up + 2 : KpU - 1;
                load_col(rT, co, pn, NE, strideB, ev2);
                __builtin_amdgcn_sched_barrier(0);
                ukn_v = F.kp_times[E0 + pn];
                __builtin_amdgcn_sched_barrier(0);
            }
            const double dt = (double)(t + 1 - uks);                       // 0 behind a crossing: the next step IS the key-point
            Ya.x = lerp_nc(sv[0], dt, av[0]); Ya.y = lerp_nc(sv[1], dt, av[1]); Ya.z = lerp_nc(sv[2], dt, av[2]); Ya.w = lerp_nc(sv[3], dt, av[3]);
            Yb.x = lerp_nc(sv[4], dt, av[4]); Yb.y = NCU > 1 ? lerp_nc(sv[5], dt, av[5]) : 0.0;
            Yb.z = NCU > 2 ? lerp_nc(sv[6], dt, av[6]) : 0.0; Yb.w = NCU > 3 ? lerp_nc(sv[7], dt, av[7]) : 0.0;
        }
        // quadratic cost model on the residuals: sum_k w_k [Jx_k (2 r_k + Jx_k) + Ju_k (2 r_k + Ju_k)]
        if constexpr (MODE == 0) {
            if (t == T - 1) {                     // terminal weights at the last step (Optimiser.cpp:209-211)
#pragma unroll
                for (int r = 0; r < 4; r++) wcur[r] = (sig(4 * r + q) < nr) ? F.w_term[sig(4 * r + q)] : 0.0;   // (hoisting these loads out of the loop measured 0.9 ms slower)
            }
        } else if constexpr (MODE == 3) {
#pragma unroll
            for (int r = 0; r < 4; r++) wcur[r] = wterm[r];
        }
        if constexpr (ROLE == 1) {                 // nothing to score, nothing to request: r belongs to the pair
        } else if constexpr (ROLE == 3) {          // scores itself, signs on the spot; r came with the requests in front of the last group
            if constexpr (MODE == 3)
                partial += sgterm[0] * (Jx.x * __builtin_fma(s2term[0], rvF.x, Jx.x)) + sgterm[1] * (Jx.y * __builtin_fma(s2term[1], rvF.y, Jx.y))
                         + sgterm[2] * (Jx.z * __builtin_fma(s2term[2], rvF.z, Jx.z)) + sgterm[3] * (Jx.w * __builtin_fma(s2term[3], rvF.w, Jx.w));
            else
                partial += sgrun[0] * (Jx.x * __builtin_fma(s2run[0], rvE.x, Jx.x)) + sgrun[1] * (Jx.y * __builtin_fma(s2run[1], rvE.y, Jx.y))
                         + sgrun[2] * (Jx.z * __builtin_fma(s2run[2], rvE.z, Jx.z)) + sgrun[3] * (Jx.w * __builtin_fma(s2run[3], rvE.w, Jx.w));
        } else if constexpr (ROLE == 2) {          // lanes c < 8: this step; lanes c >= 8: the even member, with the r of its own row
            const d4 rp = S[PAR & ~1].rv;
            acc4[0] = __builtin_fma(Jx.x, __builtin_fma(s2run[0], rp.x, Jx.x), acc4[0]);
            acc4[1] = __builtin_fma(Jx.y, __builtin_fma(s2run[1], rp.y, Jx.y), acc4[1]);
            acc4[2] = __builtin_fma(Jx.z, __builtin_fma(s2run[2], rp.z, Jx.z), acc4[2]);
            acc4[3] = __builtin_fma(Jx.w, __builtin_fma(s2run[3], rp.w, Jx.w), acc4[3]);
            __builtin_amdgcn_sched_barrier(0);
            // the pair NS steps on: rows t - 1 + NS and t + NS (behind the last pair: rows T-2, T-1, never used)
            const int sRp = (t + NS < T ? t - 1 + NS : T - 2) * nr * 8;
            double r0, r1, r2, r3;
            kp_bld2s(rR, oR2p[0], sRp, r0, r1); kp_bld2s(rR, oR2p[1], sRp, r2, r3);
            S[PAR & ~1].rv.x = r0; S[PAR & ~1].rv.y = r1; S[PAR & ~1].rv.z = r2; S[PAR & ~1].rv.w = r3;
            __builtin_amdgcn_sched_barrier(0);
        } else {
        const d4 r2 = cur.rv + cur.rv;
        if constexpr (SQW) {
            if constexpr (MODE == 3) {         // the final step: terminal weights, their signs applied on the spot
                partial += sgterm[0] * (Jx.x * __builtin_fma(s2term[0], cur.rv.x, Jx.x)) + sgterm[1] * (Jx.y * __builtin_fma(s2term[1], cur.rv.y, Jx.y))
                         + sgterm[2] * (Jx.z * __builtin_fma(s2term[2], cur.rv.z, Jx.z)) + sgterm[3] * (Jx.w * __builtin_fma(s2term[3], cur.rv.w, Jx.w));
            } else {
                acc4[0] = __builtin_fma(Jx.x, __builtin_fma(s2run[0], cur.rv.x, Jx.x), acc4[0]);
                acc4[1] = __builtin_fma(Jx.y, __builtin_fma(s2run[1], cur.rv.y, Jx.y), acc4[1]);
                acc4[2] = __builtin_fma(Jx.z, __builtin_fma(s2run[2], cur.rv.z, Jx.z), acc4[2]);
                acc4[3] = __builtin_fma(Jx.w, __builtin_fma(s2run[3], cur.rv.w, Jx.w), acc4[3]);
            }
        } else if constexpr (RU0)                      // Ju = 0 exactly: its term adds a signed zero
            partial += wcur[0] * (Jx.x * (r2.x + Jx.x)) + wcur[1] * (Jx.y * (r2.y + Jx.y))
                     + wcur[2] * (Jx.z * (r2.z + Jx.z)) + wcur[3] * (Jx.w * (r2.w + Jx.w));
        else
            partial += wcur[0] * (Jx.x * (r2.x + Jx.x) + Ju.x * (r2.x + Ju.x))
                     + wcur[1] * (Jx.y * (r2.y + Jx.y) + Ju.y * (r2.y + Ju.y))
                     + wcur[2] * (Jx.z * (r2.z + Jx.z) + Ju.z * (r2.z + Ju.z))
                     + wcur[3] * (Jx.w * (r2.w + Jx.w) + Ju.w * (r2.w + Ju.w));
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (RV2) {
            double r0, r1, r2, r3;
            kp_bld2s(rR, oR2[0], sR, r0, r1); kp_bld2s(rR, oR2[1], sR, r2, r3);
            cur.rv.x = r0; cur.rv.y = r1; cur.rv.z = r2; cur.rv.w = r3;
        } else {
        cur.rv.x = kp_blds(rR, oR[0], sR); cur.rv.y = kp_blds(rR, oR[1], sR); cur.rv.z = kp_blds(rR, oR[2], sR); cur.rv.w = kp_blds(rR, oR[3], sR);
        }
        __builtin_amdgcn_sched_barrier(0);
        }
    };
    if constexpr (UNI) {
        // Segments from the bottom: segment p = steps k_p .. k_p+1 - 1; the last key-point T-1 is a segment of its own (the
        // final step).  On entry of the loop: sv = column(k_0), ev = column(k_1), ev2 = column(k_2) in flight, av = slope of
        // segment 0, Y(0) = sv.  (The per-lane tracker above did the loads of sv and ev; it is not used any further.)
#pragma unroll
        for (int r = 0; r < 4; r++) wterm[r] = (sig(4 * r + q) < nr) ? F.w_term[sig(4 * r + q)] : 0.0;
        uks = __builtin_amdgcn_readfirstlane(F.kp_times[E0]);
        uke = __builtin_amdgcn_readfirstlane(F.kp_times[E0 + (KpU > 1 ? 1 : 0)]);
        {
            const int p2 = KpU > 2 ? 2 : KpU - 1;
            load_col(rT, co, p2, NE, strideB, ev2);
            ukn_v = F.kp_times[E0 + p2];
            const int gap = uke - uks;
            const double den = (double)(gap > 0 ? gap : 1), rinv = kp_rcp(den);
#pragma unroll
            for (int i = 0; i < 8; i++) av[i] = fdiv(ev[i] - sv[i], den, rinv);
            if (c == n || c == n + 1) {
#pragma unroll
                for (int r = 0; r < 4; r++) if (4 * r + q == c) { ev[r] = 1.0; av[r] = 0.0; }
            }
        }
        int t = 0;
        for (; t + NS < T; t += NS) fwd_steps<0, NS, 1, P2>(step, t);     // (the crossing inside a step moves up, uks, uke on)
        if constexpr (P2) {
            // What is left, 1..NS steps: pairs while two running steps remain, then step T-2 by itself if it has no partner, then the
            // final step.  The r of those two is requested here, in front of every branch, in all lanes.  Each step runs on the set
            // its tiles were requested into (set = steps past t), as (step: MODE, set, role):
            //   left = 1:                                                                T-1: 3, 0, 3
            //   left = 2:  t: 1, 0, 3 (T-2, no partner)                                  T-1: 3, 1, 3
            //   left = 3:  t: 1, 0, 1   t+1: 1, 1, 2 (T-2)                               T-1: 3, 2, 3
            //   left = 4:  t: 1, 0, 1   t+1: 1, 1, 2   t+2: 1, 2, 3 (T-2, no partner)    T-1: 3, 3, 3
            {
                const int sE = (T > 1 ? T - 2 : 0) * nr * 8, sF = (T - 1) * nr * 8;
                double r0, r1, r2, r3;
                kp_bld2s(rR, oR2[0], sE, r0, r1); kp_bld2s(rR, oR2[1], sE, r2, r3);
                rvE.x = r0; rvE.y = r1; rvE.z = r2; rvE.w = r3;
                kp_bld2s(rR, oR2[0], sF, r0, r1); kp_bld2s(rR, oR2[1], sF, r2, r3);
                rvF.x = r0; rvF.y = r1; rvF.z = r2; rvF.w = r3;
            }
            using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
            using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
            static_assert(NS == 4, "the remainder below is written for four register sets");
            const int left = T - t;
            if (left >= 3) {
                step(t, I1{}, I0{}, I1{});
                step(t + 1, I1{}, I1{}, I2{});
                if (left == 4) { step(t + 2, I1{}, I2{}, I3{}); step(T - 1, I3{}, I3{}, I3{}); }
                else step(T - 1, I3{}, I2{}, I3{});
            } else if (left == 2) { step(t, I1{}, I0{}, I3{}); step(T - 1, I3{}, I1{}, I3{}); }
            else step(T - 1, I3{}, I0{}, I3{});
        } else
        fwd_tail<0, NS, 1>(step, t, T);
    } else {
        int t = 0;
        for (; t + NS <= T; t += NS) fwd_steps<0, NS, 0>(step, t);
        fwd_tail<0, NS, 0>(step, t, T);
    }
    if constexpr (P2) {                // the even members sit in lanes c >= 8 of the pair sums (and of nothing else)
        double pairs = sgrun[0] * acc4[0] + sgrun[1] * acc4[1] + sgrun[2] * acc4[2] + sgrun[3] * acc4[3];
        pairs += __shfl_xor(pairs, 8);
        partial += pairs;
    } else
    if constexpr (SQW) partial += sgrun[0] * acc4[0] + sgrun[1] * acc4[1] + sgrun[2] * acc4[2] + sgrun[3] * acc4[3];
    partial += __shfl_xor(partial, 16);
    partial += __shfl_xor(partial, 32);
    if (q == 0 && c < n_alpha) cost_pred[(size_t)b * n_alpha + c] = partial;
}

// The one-wave forward sweep comes in two forms, launched back to back: UNI for key-point sets in which every DoF of a
// trajectory has the same list (the device flag of k_kp_uniform says so), the general form otherwise.  Each looks at the
// flag first and leaves if the set is not its kind, so the host never has to know.
// EXCL, LISTED: the trailing flags of every forward sweep kernel.  LISTED (kpilqr_forward_linear_partial): block
// i sweeps trajectory list[i] -- a scalar load off a kernel argument, so the index the per-trajectory descriptors are built from stays
// wave-uniform.  LISTED = false, the launch of every whole-batch call, never reads `list`.  (The index is formed in the call of the
// body, where the body's default argument forms the block's own: in front of it, the compiler orders the entry block differently.)
template <int NCZ, int NCU, bool RU0, bool UNI, bool RXC, bool PAIR2, bool EXCL, bool LISTED>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, EXCL ? 1 : 0)))
k_forward_fused(RecLayout L, FusedArgs F, int T, int n_alpha, const double *__restrict__ Kin,
                const double *__restrict__ kin, const double *__restrict__ u_nom, const double *__restrict__ ctrl_lim,
                const double *__restrict__ alphas, double *__restrict__ cost_pred, double *__restrict__ U_alpha,
                const int *__restrict__ kp_uniform, const int *__restrict__ list)
{
    if ((*kp_uniform != 0) != UNI) return;
    forward_fused_body<NCZ, NCU, RU0, UNI, RXC, PAIR2>(L, F, T, n_alpha, Kin, kin, u_nom, ctrl_lim, alphas, cost_pred, U_alpha,
                                                       LISTED ? list[blockIdx.x] : KP_BLOCK_TRAJ);
}

// ---------------------------------------------------------------------------------------------------------
// Forward pass, STATE / COST wave pair per trajectory (small batches: every wave has a SIMD to itself).  Only the state
// recursion is serial in time: wave S keeps Z and runs  U = u_nom + K dx + alpha k | clamp | Z' = A dx + B du  (10 MFMAs a
// step) and publishes (Z_t, dU_t); wave C, one step behind, scores the candidates (Jx = r_x dx, Ju = r_u du, the weighted
// quadratic: 6 MFMAs + the FP64 VALU work) and, one step ahead, interpolates the A, B columns of the next step (a4) into
// the transposing LDS tiles S reads.  One s_barrier per step, two ring slots each way.
#define FSC_Y 544                                 // one Y slot: A then B, [16][17] each
#define FSC_YS 0
#define FSC_ZS (2 * FSC_Y)                        // two (Z, dU) slots, D layout
#define FSC_TOTAL (FSC_ZS + 2 * 512)

// RU0: nobody reads the control change of a step (no control residuals to score): its LDS image is not written
// UNI: every DoF of the trajectory has the same key-point list -- the state wave interpolates its own operands Ya, Yb in the
// operand layout, straight from the column store (the segment tracker of forward_fused_body's UNI form: positions and times are
// wave-uniform scalars, the crossing sits behind a scalar branch at the end of a segment's last step); nobody stages columns
// through LDS, and the group needs no third wave.
template <int NCZ, int NCU, bool RU0 = false, bool UNI = false>
__device__ __forceinline__ void forward_sc_state(double *sh, RecLayout L, int T, int n_alpha, const double *__restrict__ Kin,
               const double *__restrict__ kin, const double *__restrict__ u_nom, const double *__restrict__ ctrl_lim,
               const double *__restrict__ alphas, double *__restrict__ U_alpha, const FusedArgs *Fp = nullptr, const int btraj = blockIdx.x)
{
    const int n = L.n, m = L.m;
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int b = btraj;
    int oK[4], oub[4];
    double lo[NCU], hi[NCU], kmask[4];
    // k rides in row n of the gain operand: ONE load (the lanes of that row), added into the register that holds the row
    const int okn = (q == (n & 3) && c < m) ? 8 * c : KP_OOB;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = 4 * r + q;
        oK[r] = (row < n && c < m) ? 8 * (row * m + c) : KP_OOB;
        kmask[r] = (r == (n >> 2)) ? 1.0 : 0.0;
        oub[r] = (row < m) ? 8 * row : KP_OOB;
        if (r < NCU) {
            lo[r] = (row < m) ? ctrl_lim[2 * row] : -1.0e300;
            hi[r] = (row < m) ? ctrl_lim[2 * row + 1] : 1.0e300;
        }
    }
    const double my_alpha = (c < n_alpha) ? alphas[c] : 0.0;
    d4 Z;
    {
        double zr[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 4 * r + q;
            zr[r] = (row == n) ? my_alpha : (row == n + 1) ? 1.0 : 0.0;
        }
        Z.x = zr[0]; Z.y = zr[1]; Z.z = zr[2]; Z.w = zr[3];
    }
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    // KP_FSC_SETS tile sets (step t works on set t mod KP_FSC_SETS): each is re-requested for step t + KP_FSC_SETS right behind
    // its use in step t.  The time loop is a body of KP_FSC_SETS steps WITHOUT conditions (the steps below a full group are
    // peeled behind it): a request inside `if (t + 1 < T)` makes every later wait conservative
    struct STiles { d4 YkK, ub; double kk; };
    // one descriptor per array for the whole trajectory, the step in the loads' scalar offset (behind the last step: step T-1
    // again, never used) -- as in forward_fused_body
    const __amdgpu_buffer_rsrc_t rK = kp_rsrc(Kin + (size_t)b * T * m * n, T * m * n * 8), rk = kp_rsrc(kin + (size_t)b * T * m, T * m * 8),
                                 ru = kp_rsrc(u_nom + (size_t)b * T * m, T * m * 8);
    auto request = [&](int t, STiles &s_) {
        const int tn = t < T ? t : T - 1;
        const int sK = tn * m * n * 8, sk = tn * m * 8;
        s_.YkK.x = kp_blds(rK, oK[0], sK); s_.YkK.y = kp_blds(rK, oK[1], sK); s_.YkK.z = kp_blds(rK, oK[2], sK); s_.YkK.w = kp_blds(rK, oK[3], sK);
        s_.kk = kp_blds(rk, okn, sk);
        s_.ub.x = kp_blds(ru, oub[0], sk); s_.ub.y = NCU > 1 ? kp_blds(ru, oub[1], sk) : 0.0;
        s_.ub.z = NCU > 2 ? kp_blds(ru, oub[2], sk) : 0.0; s_.ub.w = NCU > 3 ? kp_blds(ru, oub[3], sk) : 0.0;
    };
    // ---- UNI: the segment tracker (forward_fused_body) ----
    ColOffs co;
    double sv[8], ev[8], ev2[8], av[8];
    int up = 0, uks = 0, uke = 0, ukn_v = 0, E0 = 0, NE = 0, KpU = 1;
    __amdgpu_buffer_rsrc_t rT = rK;
    d4 Yua = zero, Yub = zero;                         // the operands of the NEXT step
    (void)co; (void)sv; (void)ev; (void)ev2; (void)av; (void)up; (void)uks; (void)uke; (void)ukn_v; (void)E0; (void)NE; (void)KpU; (void)rT;
    constexpr int strideBc = 0;
    (void)strideBc;
    const int strideB = 3 * n * 8;
    if constexpr (UNI) {
        const FusedArgs &F = *Fp;
        E0 = F.kp_offsets[(size_t)b * F.dof]; NE = F.kp_offsets[(size_t)(b + 1) * F.dof] - E0;
        KpU = F.kp_offsets[(size_t)b * F.dof + 1] - E0;
        rT = kp_rsrc(F.kpc + (size_t)E0 * 3 * n, NE * strideB);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            // the Y operands themselves: Ya(p = row, o = c) = A(o, p), Yb(p, o) = B(o, p) -- element c of column `row`, whose
            // DoF list starts (row mod dof) * KpU entries into the trajectory's slice
            const int row = 4 * r + q;
            const int d = row < F.dof ? row : row - F.dof;
            co.a[r] = (row < n && c < n) ? 8 * ((d * KpU * 3 + (row < F.dof ? 0 : 1)) * n + c) : BIGOFF;
            co.b[r] = (row < m && c < n) ? 8 * ((row * KpU * 3 + 2) * n + c) : BIGOFF;
        }
        load_col(rT, co, 0, NE, strideB, sv);
        load_col(rT, co, KpU > 1 ? 1 : 0, NE, strideB, ev);
        uks = __builtin_amdgcn_readfirstlane(F.kp_times[E0]);
        uke = __builtin_amdgcn_readfirstlane(F.kp_times[E0 + (KpU > 1 ? 1 : 0)]);
        const int p2 = KpU > 2 ? 2 : KpU - 1;
        load_col(rT, co, p2, NE, strideB, ev2);
        ukn_v = F.kp_times[E0 + p2];
        const int gap = uke - uks;
        const double den = (double)(gap > 0 ? gap : 1), rinv = kp_rcp(den);
#pragma unroll
        for (int i = 0; i < 8; i++) av[i] = fdiv(ev[i] - sv[i], den, rinv);
        // the identity rows of Ya (alpha and the homogeneous 1 carry over): lanes c >= n walk no list
        if (c == n || c == n + 1) {
#pragma unroll
            for (int r = 0; r < 4; r++) if (4 * r + q == c) { sv[r] = 1.0; ev[r] = 1.0; av[r] = 0.0; }
        }
        Yua.x = sv[0]; Yua.y = sv[1]; Yua.z = sv[2]; Yua.w = sv[3];            // Y(0): the first key-point is step 0
        Yub.x = sv[4]; Yub.y = NCU > 1 ? sv[5] : 0.0; Yub.z = NCU > 2 ? sv[6] : 0.0; Yub.w = NCU > 3 ? sv[7] : 0.0;
    }
    // the operands of step t + 1, formed behind the products of step t (UNI)
    auto next_Y = [&](int t) __attribute__((always_inline)) {
        const FusedArgs &F = *Fp;
        if (t + 1 == uke) {
            // crossing into segment up + 1: its start column (ev) and end column (ev2) were requested one and two segments ago;
            // the column after those and its time are requested now, the time BEHIND the columns (loads return in order)
            const int kn = __builtin_amdgcn_readfirstlane(ukn_v);
            uks = uke; uke = kn; up++;
            const int gap = uke - uks;
            const double den = (double)(gap > 0 ? gap : 1), rinv = kp_rcp(den);
#pragma unroll
            for (int i = 0; i < 8; i++) { sv[i] = ev[i]; ev[i] = ev2[i]; av[i] = fdiv(ev[i] - sv[i], den, rinv); }
            if (c == n || c == n + 1) {
#pragma unroll
                for (int r = 0; r < 4; r++) if (4 * r + q == c) { sv[r] = 1.0; ev[r] = 1.0; av[r] = 0.0; }
            }
            const int pn = up + 2 < KpU ? up + 2 : KpU - 1;
            load_col(rT, co, pn, NE, strideB, ev2);
            __builtin_amdgcn_sched_barrier(0);
            ukn_v = F.kp_times[E0 + pn];
            __builtin_amdgcn_sched_barrier(0);
        }
        const double dt = (double)(t + 1 - uks);                       // 0 behind a crossing: the next step IS the key-point
        Yua.x = lerp_nc(sv[0], dt, av[0]); Yua.y = lerp_nc(sv[1], dt, av[1]); Yua.z = lerp_nc(sv[2], dt, av[2]); Yua.w = lerp_nc(sv[3], dt, av[3]);
        Yub.x = lerp_nc(sv[4], dt, av[4]); Yub.y = NCU > 1 ? lerp_nc(sv[5], dt, av[5]) : 0.0;
        Yub.z = NCU > 2 ? lerp_nc(sv[6], dt, av[6]) : 0.0; Yub.w = NCU > 3 ? lerp_nc(sv[7], dt, av[7]) : 0.0;
    };
    auto step = [&](int t, STiles &s_) {
        const double *shA = sh + FSC_YS + (t & 1) * FSC_Y, *shB = shA + 272;
        d4 Ya, Yb;                                     // Ya(p, o) = A(o, p);  Yb(p, o) = B(o, p)
        if constexpr (UNI) { Ya = Yua; Yb = Yub; }
        else {
        Ya.x = shA[c * 17 + q];      Ya.y = shA[c * 17 + 4 + q];
        Ya.z = shA[c * 17 + 8 + q];  Ya.w = shA[c * 17 + 12 + q];
        Yb.x = shB[c * 17 + q];                Yb.y = NCU > 1 ? shB[c * 17 + 4 + q] : 0.0;
        Yb.z = NCU > 2 ? shB[c * 17 + 8 + q] : 0.0; Yb.w = NCU > 3 ? shB[c * 17 + 12 + q] : 0.0;
        }
        d4 Yk = s_.YkK;
        {
            const double kk = s_.kk;                   // (a product with the 0 / 1 mask: no branch, no select on the register index)
            Yk.x = __builtin_fma(kmask[0], kk, Yk.x); Yk.y = __builtin_fma(kmask[1], kk, Yk.y);
            Yk.z = __builtin_fma(kmask[2], kk, Yk.z); Yk.w = __builtin_fma(kmask[3], kk, Yk.w);
        }
        const d4 ub = s_.ub;
        d4 U = kp_P<NCZ>(Yk, Z, ub);                     // u_nom + K dx + alpha k   (:879)
        __builtin_amdgcn_sched_barrier(0);
        request(t + KP_FSC_SETS, s_);
        __builtin_amdgcn_sched_barrier(0);
        d4 Zn = kp_P<NCZ>(Ya, Z, zero);                  // A dx
        d4 dU = zero;
        {
            double u;                                  // clamp (:883-889)
            u = U.x; if (u > hi[0]) u = hi[0]; if (u < lo[0]) u = lo[0]; U.x = u; dU.x = u - ub.x;
            if (NCU > 1) { u = U.y; if (u > hi[1]) u = hi[1]; if (u < lo[1]) u = lo[1]; U.y = u; dU.y = u - ub.y; }
            if (NCU > 2) { u = U.z; if (u > hi[2]) u = hi[2]; if (u < lo[2]) u = lo[2]; U.z = u; dU.z = u - ub.z; }
            if (NCU > 3) { u = U.w; if (u > hi[3]) u = hi[3]; if (u < lo[3]) u = lo[3]; U.w = u; dU.w = u - ub.w; }
        }
        double *zs = sh + FSC_ZS + (t & 1) * 512;
        kp_lds_store(zs, lane, Z);                       // the state this step started from, and its control change
        if constexpr (!RU0) kp_lds_store(zs + 256, lane, dU);
        Z = kp_P<NCU>(Yb, dU, Zn);                       // + B du: the next state
        if (U_alpha && c < n_alpha) {
            double *Ua = U_alpha + (((size_t)b * n_alpha + c) * T + t) * m;
            const double uv[4] = {U.x, U.y, U.z, U.w};
#pragma unroll
            for (int r = 0; r < NCU; r++) { const int row = 4 * r + q; if (row < m) Ua[row] = uv[r]; }
        }
        if constexpr (UNI) next_Y(t);                  // a4 of step t+1 under the products above
        __syncthreads();
    };
    STiles S[KP_FSC_SETS];
#pragma unroll
    for (int k = 0; k < KP_FSC_SETS; k++) request(k, S[k]);
    __syncthreads();                                   // Y(0) is staged
    int t = 0;
    for (; t + KP_FSC_SETS <= T; t += KP_FSC_SETS) {
#pragma unroll
        for (int k = 0; k < KP_FSC_SETS; k++) step(t + k, S[k]);
    }
#pragma unroll
    for (int k = 0; k < KP_FSC_SETS - 1; k++) if (t + k < T) step(t + k, S[k]);
}

// ROLE 1: score only (the cost wave); 2: stage the A, B columns only (third wave of the triple)
// RU0: r_u = 0 (no r_u tiles, no Ju product); RXC (with RU0): ONE constant r_x, its transposed tile in registers (forward_fused_body)
template <int NCZ, int NCU, int ROLE, bool RU0 = false, bool RXC = false>
__device__ __forceinline__ void forward_sc_cost(double *sh, RecLayout L, FusedArgs F, int T, int n_alpha, double *__restrict__ cost_pred, const int btraj = blockIdx.x)
{
    const int n = L.n, m = L.m;
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int b = btraj;
    const int nr = F.nr;
    const int strideB = 3 * L.n * 8;                               // bytes of one key-point entry of kpc: three columns
    const int ncx = (n + 3) >> 2;
    ColOffs co;
    col_offsets(co, n, m, F.dof, c, q);
    int oRxT[4], oRuT[4], oR[4];
    double wcur[4], wterm[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = 4 * r + q;
        oRxT[r] = (row < n && c < nr) ? 8 * (c * n + row) : KP_OOB;     // RxT(p=row, k=c) = r_x[k][p]
        oRuT[r] = (row < m && c < nr) ? 8 * (c * m + row) : KP_OOB;     // RuT(p=row, k=c) = r_u[k][p]
        oR[r] = (row < nr) ? 8 * row : KP_OOB;
        wcur[r] = (row < nr) ? F.w_run[row] : 0.0;
        wterm[r] = (row < nr) ? F.w_term[row] : 0.0;   // in registers from the start: a load inside the time loop makes the
                                                       // compiler drain every outstanding prefetch (vmcnt(0)) each step here
    }
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    double partial = 0.0;
    const int E0 = F.kp_offsets[(size_t)b * F.dof], NE = F.kp_offsets[(size_t)(b + 1) * F.dof] - E0;      // this trajectory's key-point entries
    __amdgpu_buffer_rsrc_t rT = kp_rsrc(F.kpc + (size_t)E0 * 3 * L.n, NE * strideB);
    const double *rb = F.r + (size_t)b * (T + 1) * nr;
    const double *rxb = F.r_x + (size_t)b * (T + 1) * nr * n;
    const double *rub = F.r_u + (size_t)b * (T + 1) * nr * m;
    struct CTiles { d4 RxT, RuT, rv; };
    const __amdgpu_buffer_rsrc_t rNone = kp_rsrc(rb, 0);
    d4 RxTc = {0.0, 0.0, 0.0, 0.0};
    if constexpr (RXC) {
        __amdgpu_buffer_rsrc_t rRxc = kp_rsrc(F.rx_const, nr * n * 8);
        RxTc.x = kp_bld(rRxc, oRxT[0]); RxTc.y = kp_bld(rRxc, oRxT[1]); RxTc.z = kp_bld(rRxc, oRxT[2]); RxTc.w = kp_bld(rRxc, oRxT[3]);
    }
    (void)RxTc;
    auto request = [&](int t, CTiles &s_) {
        const bool ok = t < T;
        __amdgpu_buffer_rsrc_t rRx = ok ? kp_rsrc(rxb + (size_t)t * nr * n, nr * n * 8) : rNone;
        __amdgpu_buffer_rsrc_t rRu = ok ? kp_rsrc(rub + (size_t)t * nr * m, nr * m * 8) : rNone;
        __amdgpu_buffer_rsrc_t rR = ok ? kp_rsrc(rb + (size_t)t * nr, nr * 8) : rNone;
        if constexpr (!RXC) { s_.RxT.x = kp_bld(rRx, oRxT[0]); s_.RxT.y = kp_bld(rRx, oRxT[1]); s_.RxT.z = kp_bld(rRx, oRxT[2]); s_.RxT.w = kp_bld(rRx, oRxT[3]); }
        if constexpr (!RU0) {
            s_.RuT.x = kp_bld(rRu, oRuT[0]); s_.RuT.y = NCU > 1 ? kp_bld(rRu, oRuT[1]) : 0.0;
            s_.RuT.z = NCU > 2 ? kp_bld(rRu, oRuT[2]) : 0.0; s_.RuT.w = NCU > 3 ? kp_bld(rRu, oRuT[3]) : 0.0;
        }
        s_.rv.x = kp_bld(rR, oR[0]); s_.rv.y = kp_bld(rR, oR[1]); s_.rv.z = kp_bld(rR, oR[2]); s_.rv.w = kp_bld(rR, oR[3]);
    };
    // ---- column tracker, walking UP in time (as in forward_fused_body) ----
    const int kd = (c < F.dof) ? c : c - F.dof;
    const bool has = c < n;
    const int klo = has ? F.kp_offsets[(size_t)b * F.dof + kd] : 0;
    const int khi = has ? F.kp_offsets[(size_t)b * F.dof + kd + 1] : 0;
    int idx = klo;
    int s = has ? F.kp_times[idx] : 0;
    int e = (has && idx + 1 < khi) ? F.kp_times[idx + 1] : BIGT;
    int nb = (has && idx + 2 < khi) ? F.kp_times[idx + 2] : BIGT;
    double sv[8], ev[8], av[8];
    if (ROLE == 2) {
        load_col(rT, co, has ? idx - E0 : -1, NE, strideB, sv);
        load_col(rT, co, (has && idx + 1 < khi) ? idx + 1 - E0 : -1, NE, strideB, ev);
    }
    bool pend = true;
#pragma unroll
    for (int i = 0; i < 8; i++) av[i] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++) if ((c == n || c == n + 1) && 4 * r + q == c) sv[r] = 1.0;
    auto stage_cols = [&](int t) {
        double *shA = sh + FSC_YS + (t & 1) * FSC_Y, *shB = shA + 272;
        const double dt = (double)(t - s);
        shA[(q) * 17 + c] = lerp_nc(sv[0], dt, av[0]);      shA[(4 + q) * 17 + c] = lerp_nc(sv[1], dt, av[1]);
        shA[(8 + q) * 17 + c] = lerp_nc(sv[2], dt, av[2]);  shA[(12 + q) * 17 + c] = lerp_nc(sv[3], dt, av[3]);
        shB[(q) * 17 + c] = lerp_nc(sv[4], dt, av[4]);      shB[(4 + q) * 17 + c] = lerp_nc(sv[5], dt, av[5]);
        shB[(8 + q) * 17 + c] = lerp_nc(sv[6], dt, av[6]);  shB[(12 + q) * 17 + c] = lerp_nc(sv[7], dt, av[7]);
    };
    auto advance = [&](int t) {
        if (pend) {
            const double den = (double)(e - s);
            const double rinv = kp_rcp(den);
#pragma unroll
            for (int i = 0; i < 8; i++) av[i] = (e != BIGT) ? fdiv(ev[i] - sv[i], den, rinv) : 0.0;
            pend = false;
        }
        if (t >= e) {
#pragma unroll
            for (int i = 0; i < 8; i++) { sv[i] = ev[i]; av[i] = 0.0; }
            s = e; e = nb; idx++;
            load_col(rT, co, (idx + 1 < khi) ? idx + 1 - E0 : -1, NE, strideB, ev);
            nb = (idx + 2 < khi) ? F.kp_times[idx + 2] : BIGT;
            pend = true;
        }
    };
    // iteration t: score step t-1 (tiles re-requested for step t+1 right behind their use), then stage the A, B columns of
    // step t+1 for wave S
    auto iter = [&](int t, CTiles &s_) {               // s_ holds the tiles of step t-1
        if (ROLE == 1 && t >= 1) {
            const int tt = t - 1;
            const double *zs = sh + FSC_ZS + (tt & 1) * 512;
            const d4 Zt = kp_lds_tile(zs, lane);
            d4 Ju = zero;                              // RU0: the control residual term vanishes (and nobody reads the dU slot)
            if constexpr (!RU0) { const d4 dU = kp_lds_tile(zs + 256, lane); Ju = kp_P<NCU>(s_.RuT, dU, zero); }
            const d4 Jx = kp_Pn(RXC ? RxTc : s_.RxT, Zt, zero, ncx);
            const d4 r2 = s_.rv + s_.rv;
            __builtin_amdgcn_sched_barrier(0);
            request(tt + KP_FSC_SETS, s_);
            __builtin_amdgcn_sched_barrier(0);
            if (tt == T - 1) {                // terminal weights at the last step (Optimiser.cpp:209-211)
#pragma unroll
                for (int r = 0; r < 4; r++) wcur[r] = wterm[r];
            }
            // sum_k w_k [Jx_k (2 r_k + Jx_k) + Ju_k (2 r_k + Ju_k)]
            if constexpr (RU0)                         // (Ju = 0 exactly: its term adds a signed zero, as in forward_fused_body)
                partial += wcur[0] * (Jx.x * (r2.x + Jx.x)) + wcur[1] * (Jx.y * (r2.y + Jx.y))
                         + wcur[2] * (Jx.z * (r2.z + Jx.z)) + wcur[3] * (Jx.w * (r2.w + Jx.w));
            else
            partial += wcur[0] * (Jx.x * (r2.x + Jx.x) + Ju.x * (r2.x + Ju.x))
                     + wcur[1] * (Jx.y * (r2.y + Jx.y) + Ju.y * (r2.y + Ju.y))
                     + wcur[2] * (Jx.z * (r2.z + Jx.z) + Ju.z * (r2.z + Ju.z))
                     + wcur[3] * (Jx.w * (r2.w + Jx.w) + Ju.w * (r2.w + Ju.w));
        }
        if (ROLE == 2 && t + 1 < T) { advance(t + 1); stage_cols(t + 1); }
        if (t < T) __syncthreads();
    };
    CTiles S[KP_FSC_SETS];                             // set k: the steps congruent k mod KP_FSC_SETS
    if (ROLE == 1) {
#pragma unroll
        for (int k = 0; k < KP_FSC_SETS; k++) request(k, S[k]);
    }
    if (ROLE == 2) stage_cols(0);
    __syncthreads();
    iter(0, S[KP_FSC_SETS - 1]);                       // (scores nothing: stages the columns of step 1)
    int t = 1;
    for (; t + KP_FSC_SETS - 1 <= T; t += KP_FSC_SETS) {   // iteration t scores step t-1, whose tiles are in set (t-1) mod KP_FSC_SETS
#pragma unroll
        for (int k = 0; k < KP_FSC_SETS; k++) iter(t + k, S[k]);
    }
#pragma unroll
    for (int k = 0; k < KP_FSC_SETS - 1; k++) if (t + k <= T) iter(t + k, S[k]);
    partial += __shfl_xor(partial, 16);
    partial += __shfl_xor(partial, 32);
    if (ROLE == 1 && q == 0 && c < n_alpha) cost_pred[(size_t)b * n_alpha + c] = partial;
}

// UNIFORM key-point sets: state wave (with its own a4) + scoring wave -- no staging wave, whatever the batch up to #SIMDs / 2.
// Leaves at once if the device flag says the set is not uniform (the general forms are launched behind it and look at the same flag).
// LISTED (see k_forward_fused; always exclusive, so no EXCL flag): every wave of block i works on trajectory list[i].
template <int NCZ, int NCU, bool RU0, bool RXC, bool LISTED>
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_forward_fused_scu(RecLayout L, FusedArgs F, int T, int n_alpha, const double *__restrict__ Kin,
                    const double *__restrict__ kin, const double *__restrict__ u_nom, const double *__restrict__ ctrl_lim,
                    const double *__restrict__ alphas, double *__restrict__ cost_pred, double *__restrict__ U_alpha,
                    const int *__restrict__ kp_uniform, const int *__restrict__ list)
{
    __shared__ __attribute__((aligned(16))) double sh[FSC_TOTAL];
    if (*kp_uniform == 0) return;
    const int listed = LISTED ? list[blockIdx.x] : 0;       // (one load in front of the role split; the block's own index is read by the role that uses it)
    const bool state = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0;
    if (state) forward_sc_state<NCZ, NCU, RU0, true>(sh, L, T, n_alpha, Kin, kin, u_nom, ctrl_lim, alphas, U_alpha, &F, LISTED ? listed : (int)blockIdx.x);
    else       forward_sc_cost<NCZ, NCU, 1, RU0, RXC>(sh, L, F, T, n_alpha, cost_pred, LISTED ? listed : (int)blockIdx.x);
}

// state + cost + staging waves (4 x batch <= #SIMDs: one 3-wave workgroup per CU): a cost wave that also stages is the longer
// one of a pair (1 360 vs 1 130 cycles per step), so its a4 half goes to a third wave
template <int NCZ, int NCU, bool RU0, bool RXC, bool LISTED>
__global__ void __launch_bounds__(192) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_forward_fused_sc3(RecLayout L, FusedArgs F, int T, int n_alpha, const double *__restrict__ Kin,
                    const double *__restrict__ kin, const double *__restrict__ u_nom, const double *__restrict__ ctrl_lim,
                    const double *__restrict__ alphas, double *__restrict__ cost_pred, double *__restrict__ U_alpha,
                    const int *__restrict__ kp_uniform, int only_ragged, const int *__restrict__ list)
{
    __shared__ __attribute__((aligned(16))) double sh[FSC_TOTAL];
    if (only_ragged && *kp_uniform != 0) return;       // (launched behind k_forward_fused_scu, which has run the uniform set)
    const int listed = LISTED ? list[blockIdx.x] : 0;       // (as in k_forward_fused_scu)
    const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (role == 0) forward_sc_state<NCZ, NCU, RU0>(sh, L, T, n_alpha, Kin, kin, u_nom, ctrl_lim, alphas, U_alpha, nullptr, LISTED ? listed : (int)blockIdx.x);
    else if (role == 1) forward_sc_cost<NCZ, NCU, 1, RU0, RXC>(sh, L, F, T, n_alpha, cost_pred, LISTED ? listed : (int)blockIdx.x);
    else forward_sc_cost<NCZ, NCU, 2>(sh, L, F, T, n_alpha, cost_pred, LISTED ? listed : (int)blockIdx.x);
}

#if KP_PART(1)
bool fused_supported(int n, int m, int nr, int dof, int T, int n_alpha)
{
    // one trajectory's slice of the key-point column store (at most T entries per DoF, 3n doubles each) behind one descriptor
    return kp_t1_shape(n, m) && nr >= 1 && nr <= 16 && m <= dof && n_alpha <= 16 && (long long)T * dof * (6 * n + 2) * 8 < (long long)BIGOFF;
}

#endif
static FusedArgs fused_args(const Ctx *c)
{
    FusedArgs F = {c->kp_offsets, c->kp_times, c->r, c->r_x, c->r_u, c->w_run, c->w_term, c->d.dof, c->d.nr,
                   c->kpc, c->fdk_dev, 2 * c->eps, 1.0 / (2 * c->eps), c->rx_const,
                   c->kps ? c->kps : c->kpc};      // (no slope store: lists known uniform, no general form runs -- never a null descriptor)
    return F;
}

#if KP_PART(1)
// ---- the plans: WHAT a fused sweep launch is (FusedLaunch, common.h).  The launchers below map a plan to kernels and decide nothing.
// Backward.  While a trajectory can have two SIMDs (2 x batch <= #SIMDs) the consumer / helper pair runs it: the consumer's chain is
// Tu | Quu | refresh | gains | V', the helper forms the side products Tz, Quz, Qzz, then a4 + a6 of the next step, and differences
// the payload of uniform sets.  Beyond that two waves take turns on a SIMD and one wave per trajectory wins.
// Both have RAW instantiations.  KPILQR_FUSED_WAVES = 1 (one wave) | 5 (the pair) forces one (diagnostic, include/kpilqr.h); any
// other value is the library's choice.  Rounds 2-4 also had a control / state split, a producer / consumer pair and a consumer /
// side / producer triple: all measured slower than the helper pair at every batch size (profiles/r04_helper_pair.txt) and were
// removed in round 5 (DESIGN_HISTORY.md keeps their numbers).
FusedLaunch plan_backward_fused(const Ctx *c, bool raw)
{
    const int f = c->tune.fused_bwd_waves;
    FusedLaunch p;
    p.waves = p.waves_ragged = f == 1 ? Waves::w1 : (f == 5 || 2 * c->d.batch <= c->n_simd) ? Waves::pairh : Waves::w1;
    p.raw = raw;
    p.ru0 = c->ru_zero;
    p.rxc = c->ru_zero && c->rx_const_on;       // (the constant-Jacobian kernels exist with r_u = 0 only)
    // per-DoF lists walk the slope store (made by k_fd_kp_difference / k_kp_slopes for such sets only) -- but for the GENERAL raw
    // form of the one-wave sweep (KPILQR_FUSED_UNI=0, diagnostic), which differences every set itself and divides at its crossings
    p.slopes = c->kps != nullptr && !(p.waves == Waves::w1 && raw && c->tune.fused_uni == 0);
    p.excl = c->d.batch <= c->n_simd;
    return p;
}

// Forward.  While 2 x batch <= #SIMDs the state / cost pair runs UNIFORM key-point sets -- the state wave interpolates its own
// operands, no staging wave -- with the state / cost / staging triple (4 x batch <= #SIMDs) or the one-wave general form behind it
// for per-DoF lists; the device flag decides which of the two runs.  Beyond that one wave per trajectory, its tile requests four
// steps ahead.  Late round 4, with r_u = 0 / constant-r_x instantiations of the scoring wave and a state wave that issues 7 loads
// per step instead of 10 (profiles/r04_forward_forms.txt): 1.31 / 1.43 / 1.47 ms at 1 / 64 / 256 trajectories (one wave per
// trajectory: 1.72; the triple alone: 1.58 at B = 1, 1.74 ... 1.76 at B = 128 ... 256).  KPILQR_FUSED_FWD_WAVES = 1 (one wave) |
// 3 (triple) | 4 (pair) forces one (diagnostic, include/kpilqr.h); any other value is the library's choice.
FusedLaunch plan_forward_fused(const Ctx *c)
{
    const int f = c->tune.fused_fwd_waves;
    FusedLaunch p;
    p.waves = f == 1 ? Waves::w1 : f == 3 ? Waves::triple : (f == 4 || 2 * c->d.batch <= c->n_simd) ? Waves::pair : Waves::w1;
    p.waves_ragged = p.waves != Waves::pair ? p.waves : 4 * c->d.batch <= c->n_simd ? Waves::triple : Waves::w1;
    p.ru0 = c->ru_zero;
    p.rxc = c->ru_zero && c->rx_const_on;       // (every form's cost wave has its constant-Jacobian instantiation, with r_u = 0 only)
    p.slopes = p.waves_ragged == Waves::w1 && c->kps != nullptr;
    p.excl = c->d.batch <= c->n_simd;
    // the uniform one-wave form with the constant Jacobian scores two steps per r_x product while the candidates fill at most half
    // of the tile's columns (forward_fused_body, P2)
    p.pair2 = p.waves == Waves::w1 && p.rxc && c->d.n_alpha <= 8;
    return p;
}

// ---- one wave per trajectory, backward
template <int NN, int MM, bool RU, bool RW, bool UN, bool RX>
static void launch_bf_kernel(Ctx *c, const FusedLaunch &p, const FusedArgs &F, int pd_stride)
{
    kp_with_flags(p.excl, c->bwd_gate != nullptr, [&](auto excl, auto gated) {
        hipLaunchKernelGGL((k_backward_fused<NN, MM, RU, RW, UN, RX, excl(), gated()>), dim3(c->d.batch), dim3(64), 0, c->stream, c->L, F,
                           c->d.T, c->lambda, pd_stride, c->K, c->k, c->delta_J, c->status, c->kp_uniform, c->bwd_gate, c->sweep_list);
    });
}
// rxc: constant residual Jacobians.  The kernels exist with r_u = 0 only, hence RX = RU: nothing is compiled for <RU = false, RX = true>
template <int NN, int MM, bool RU, bool RW, bool UN>
static void launch_bf_form(Ctx *c, const FusedLaunch &p, const FusedArgs &F, int pd_stride)
{
    if (RU && p.rxc) launch_bf_kernel<NN, MM, RU, RW, UN, RU>(c, p, F, pd_stride);
    else launch_bf_kernel<NN, MM, RU, RW, UN, false>(c, p, F, pd_stride);
}
// The launch sequence: the uniform and the general form back to back, the one whose kind of key-point set is not resident leaves
// at once.  raw: only UNIFORM sets are differenced inside the sweep; for per-DoF lists a lane's crossing is a divergent branch that
// every lane of the wave pays for (17 loads, 8 stores on most steps), and the streaming kernel + the plain general sweep are faster
// (iterative-error lists with a key-point on 99 % of the steps: 8.7 + 2.2 against 11.9 ms) -- k_fd_kp_difference is launched in
// between and looks at the same device flag.  (KPILQR_FUSED_UNI=0, diagnostic: the general form alone, raw or not, for every set.)
template <int NN, int MM, bool RU>
static hipError_t launch_bf_sequence(Ctx *c, const FusedLaunch &p, const FusedArgs &F, int pd_stride)
{
    const bool uni = c->tune.fused_uni != 0;
    if (p.raw && uni) {
        launch_bf_form<NN, MM, RU, true, true>(c, p, F, pd_stride);
        const hipError_t e = launch_fd_kp_difference(c, true);     // (per-DoF lists: columns and their slopes)
        if (e != hipSuccess) return e;
        launch_bf_form<NN, MM, RU, false, false>(c, p, F, pd_stride);
    } else if (p.raw) launch_bf_form<NN, MM, RU, true, false>(c, p, F, pd_stride);
    else {
        if (uni) launch_bf_form<NN, MM, RU, false, true>(c, p, F, pd_stride);
        launch_bf_form<NN, MM, RU, false, false>(c, p, F, pd_stride);
    }
    return hipGetLastError();
}

hipError_t launch_backward_fused(Ctx *c, const FusedLaunch &p, int pd_stride)
{
    if (p.waves == Waves::pairh) return launch_backward_fused_pair(c, p, pd_stride);
    const int n = c->n, m = c->d.m;
    const FusedArgs F = fused_args(c);
#define KP_X(NN, MM) if (n == NN && m == MM) return p.ru0 ? launch_bf_sequence<NN, MM, true>(c, p, F, pd_stride) : launch_bf_sequence<NN, MM, false>(c, p, F, pd_stride);
    KP_T1_SHAPES(KP_X)
#undef KP_X
    return hipErrorInvalidValue;
}
#endif

#if KP_PART(2)
// ---- the consumer / helper pair, backward.  guard: which kind of key-point set a launch serves (-1 any, 1 uniform, 0 per-DoF lists)
template <int NN, int MM, bool RW, bool SL>
static void launch_bph_kernel(Ctx *c, const FusedLaunch &p, const FusedArgs &F, int pd_stride, int guard)
{
    const auto pick = [&](auto gated) {
        auto kernel = k_backward_fusedph<NN, MM, RW, true, true, SL, gated()>;
        if (!p.rxc) kernel = p.ru0 ? k_backward_fusedph<NN, MM, RW, true, false, SL, gated()> : k_backward_fusedph<NN, MM, RW, false, false, SL, gated()>;
        return kernel;
    };
    hipLaunchKernelGGL(c->bwd_gate ? pick(std::true_type{}) : pick(std::false_type{}), dim3(c->d.batch), dim3(128), 0, c->stream, c->L, F,
                       c->d.T, c->tune.role_shift, c->lambda, pd_stride, c->K, c->k, c->delta_J, c->status, c->kp_uniform, guard, c->bwd_gate,
                       c->sweep_list);
}
// Per-DoF lists: the helper walks the slope store, uniform sets the column store with its dividing tracker: two launches, the
// device flag decides.  raw: the helper differences the payload of uniform sets; k_fd_kp_difference and the plain sweep behind it
// serve per-DoF lists.
template <int NN, int MM>
static hipError_t launch_bph_sequence(Ctx *c, const FusedLaunch &p, const FusedArgs &F, int pd_stride)
{
    if (p.raw) {
        launch_bph_kernel<NN, MM, true, false>(c, p, F, pd_stride, 1);
        const hipError_t e = launch_fd_kp_difference(c, true);
        if (e != hipSuccess) return e;
        if (p.slopes) launch_bph_kernel<NN, MM, false, true>(c, p, F, pd_stride, 0);
        else launch_bph_kernel<NN, MM, false, false>(c, p, F, pd_stride, 0);
    } else if (p.slopes) {
        launch_bph_kernel<NN, MM, false, false>(c, p, F, pd_stride, 1);
        launch_bph_kernel<NN, MM, false, true>(c, p, F, pd_stride, 0);
    } else launch_bph_kernel<NN, MM, false, false>(c, p, F, pd_stride, -1);
    return hipGetLastError();
}

hipError_t launch_backward_fused_pair(Ctx *c, const FusedLaunch &p, int pd_stride)
{
    const int n = c->n, m = c->d.m;
    const FusedArgs F = fused_args(c);
#define KP_X(NN, MM) if (n == NN && m == MM) return launch_bph_sequence<NN, MM>(c, p, F, pd_stride);
    KP_T1_SHAPES(KP_X)
#undef KP_X
    return hipErrorInvalidValue;
}
#endif

#if KP_PART(1)
// diagnostic: the one-wave sweep (general form, reads kpc) with the refresh histogram
hipError_t launch_backward_fused_stats(Ctx *c, int pd_stride, int *hist_dev)
{
    const int n = c->n, m = c->d.m;
    const FusedArgs F = fused_args(c);
#define KP_X(NN, MM) if (n == NN && m == MM) { hipLaunchKernelGGL((k_backward_fused_stats<NN, MM>), dim3(c->d.batch), dim3(64), 0, c->stream, c->L, F, c->d.T, c->lambda, pd_stride, c->K, c->k, c->delta_J, c->status, hist_dev); return hipGetLastError(); }
    KP_T1_SHAPES(KP_X)
#undef KP_X
    return hipErrorInvalidValue;
}

#endif
#if KP_PART(3)
// ---- forward.  Every kernel takes the same arguments (the triple one more in front of the list: only_ragged)
template <class Kernel, class... More>
static void launch_ff_kernel(Kernel kernel, int block, Ctx *c, const FusedArgs &F, double *U_alpha_dev, More... more)
{
    hipLaunchKernelGGL(kernel, dim3(c->d.batch), dim3(block), 0, c->stream, c->L, F, c->d.T, c->d.n_alpha, c->K, c->k, c->u_nom, c->ctrl_lim,
                       c->alphas, c->cost_pred, U_alpha_dev, c->kp_uniform, more..., c->sweep_list);
}
// the state / cost pair (uniform sets) and the state / cost / staging triple: the cost wave has the residual instantiations;
// a listed subset (kpilqr_forward_linear_partial) runs the LISTED instantiation of the same form
template <int NCZ, int NCU>
static void launch_ff_pair(Ctx *c, const FusedLaunch &p, const FusedArgs &F, double *U_alpha_dev)
{
    const auto pick = [&](auto listed) {
        auto kernel = k_forward_fused_scu<NCZ, NCU, true, true, listed()>;
        if (!p.rxc) kernel = p.ru0 ? k_forward_fused_scu<NCZ, NCU, true, false, listed()> : k_forward_fused_scu<NCZ, NCU, false, false, listed()>;
        return kernel;
    };
    launch_ff_kernel(c->sweep_list ? pick(std::true_type{}) : pick(std::false_type{}), 128, c, F, U_alpha_dev);
}
template <int NCZ, int NCU>
static void launch_ff_triple(Ctx *c, const FusedLaunch &p, const FusedArgs &F, double *U_alpha_dev, int only_ragged)
{
    const auto pick = [&](auto listed) {
        auto kernel = k_forward_fused_sc3<NCZ, NCU, true, true, listed()>;
        if (!p.rxc) kernel = p.ru0 ? k_forward_fused_sc3<NCZ, NCU, true, false, listed()> : k_forward_fused_sc3<NCZ, NCU, false, false, listed()>;
        return kernel;
    };
    launch_ff_kernel(c->sweep_list ? pick(std::true_type{}) : pick(std::false_type{}), 192, c, F, U_alpha_dev, only_ragged);
}
// One wave per trajectory: the uniform and the general form back to back, the one whose kind of key-point set is not resident
// leaves at once (k_forward_fused); behind the pair the general form alone.  RX = RU as in launch_bf_form.  RU (r_u never
// uploaded): the instantiation without the r_u loads and the Ju product.  Round-2 history: it measured SLOWER at first (3.76 vs
// 3.22 ms at B = 1024: the compiler's wait placement left the latency shadow it sat in), and faster once the uniform-key-point
// form and the per-trajectory descriptors had changed the loop (2.81 vs 3.03 ms).
template <int NCZ, int NCU, bool RU, bool UNI>
static void launch_ff_form(Ctx *c, const FusedLaunch &p, const FusedArgs &F, double *U_alpha_dev)
{
    kp_with_flags(p.excl, c->sweep_list != nullptr, [&](auto excl, auto listed) {
        // paired scoring (FusedLaunch::pair2): the uniform constant-Jacobian form with ONE scoring product per two steps
        if constexpr (RU && UNI) {
            if (p.rxc && p.pair2) {
                launch_ff_kernel(k_forward_fused<NCZ, NCU, true, true, true, true, excl(), listed()>, 64, c, F, U_alpha_dev);
                return;
            }
        }
        if (RU && p.rxc) launch_ff_kernel(k_forward_fused<NCZ, NCU, RU, UNI, RU, false, excl(), listed()>, 64, c, F, U_alpha_dev);
        else launch_ff_kernel(k_forward_fused<NCZ, NCU, RU, UNI, false, false, excl(), listed()>, 64, c, F, U_alpha_dev);
    });
}
template <int NCZ, int NCU, bool RU>
static void launch_ff_w1(Ctx *c, const FusedLaunch &p, const FusedArgs &F, double *U_alpha_dev, bool only_ragged)
{
    if (!only_ragged) launch_ff_form<NCZ, NCU, RU, true>(c, p, F, U_alpha_dev);
    launch_ff_form<NCZ, NCU, RU, false>(c, p, F, U_alpha_dev);
}

// The launch sequence.  The pair serves uniform sets; what runs behind it (only_ragged) leaves at once on one, and is not launched
// at all when the host placed the lists and saw them equal.
hipError_t launch_forward_fused(Ctx *c, const FusedLaunch &p, double *U_alpha_dev)
{
    if (!kp_t1_shape(c->n, c->d.m)) return hipErrorInvalidValue;
    const int ncz = (c->n + 2 + 3) / 4, ncu = (c->d.m + 3) / 4;       // tile chunks of [dx; alpha; 1] and of the controls name the shape
    const FusedArgs F = fused_args(c);
    const bool only_ragged = p.waves == Waves::pair;
#define KP_FWD_SHAPES(X) X(4, 2) X(2, 1) X(4, 1) X(3, 1)
    if (only_ragged) {
#define KP_X(NCZ, NCU) if (ncz == NCZ && ncu == NCU) launch_ff_pair<NCZ, NCU>(c, p, F, U_alpha_dev);
        KP_FWD_SHAPES(KP_X)
#undef KP_X
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess || c->kp_known_uniform) return e;
    }
    if (p.waves_ragged == Waves::triple) {
#define KP_X(NCZ, NCU) if (ncz == NCZ && ncu == NCU) launch_ff_triple<NCZ, NCU>(c, p, F, U_alpha_dev, only_ragged);
        KP_FWD_SHAPES(KP_X)
#undef KP_X
    } else {
#define KP_X(NCZ, NCU) if (ncz == NCZ && ncu == NCU) { if (p.ru0) launch_ff_w1<NCZ, NCU, true>(c, p, F, U_alpha_dev, only_ragged); else launch_ff_w1<NCZ, NCU, false>(c, p, F, U_alpha_dev, only_ragged); }
        KP_FWD_SHAPES(KP_X)
#undef KP_X
    }
#undef KP_FWD_SHAPES
    return hipGetLastError();
}
#endif

}  // namespace kpilqr
