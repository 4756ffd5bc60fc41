// svr.hip -- iLQR_SVR::LeastImportantDofs, singular-vector branch (src/Optimiser/iLQR_SVR.cpp:902-950), on the resident gains:
//   sums[b][i] = ( sum over t = 0, s, 2s, ... < T  and the min(3, m) leading singular triplets k of K[t] = U S V'  of
//                  |V(i, k) s_k| + |V(i + dof, k) s_k| ) / T
// The arithmetic is host/SVR.cpp's (ThinSVD, DofImportance) restated operation for operation: one-sided cyclic Jacobi on
// W = K[t]' (n x m), pairs (p < q) in the host's order, the same skip test, rotation, stopping rule (off < 1e-15 or 60 sweeps),
// column norms as singular values, the stable descending order, terms formed as |(W(j,i) / s_i) s_i|.
//
// Two passes per chunk of sampled steps:
//   1. one SVD per (trajectory, sampled step), writing the step's 2 * lead terms of every DoF to the staging buffer
//        stage [b][tc][2k + h][dof]   (k: rank of the triplet, h: 0 position column i, 1 velocity column i + dof);
//   2. one thread per (trajectory, DoF) adds them t-major, then k, then h -- the host's order -- onto the running sums.
// A trajectory's sums therefore depend neither on its batch neighbours nor on the chunking.  Two forms of pass 1, chosen by
// shape:
//   A  (n <= 16, n * m' <= 128, m' = m rounded up to a power of two): a lane per sampled step, W in VGPRs, the kernel
//      templated on (n, m') with the pair loops unrolled; the dot products run sequentially in the lane, as on the host, so
//      the sums are the host's bit for bit.  Pairs with q >= m are skipped by a wave-uniform test, padded columns stay 0.
//   B  (every other shape): a wave per sampled step, W column-major in LDS (each lane only ever touches its own rows), the
//      three dot products of a pair summed across the wave by an xor butterfly.  Every lane ends the butterfly with the same
//      bits (each level adds the same two partials, and addition commutes), so the rotation and the stopping test are
//      wave-uniform.  The order of the dot products' additions is not the host's: the sums agree to rounding, not bitwise.
//
// Compiled with -ffp-contract=off: no product below may be fused into an add; sqrt and the divisions are IEEE (correctly
// rounded) as on the host.
#include "common.h"

namespace kpilqr {

// host/SVR.cpp:18-28 on one column pair, given its three dot products: false = skip the pair.  off as std::max.
__device__ __forceinline__ bool jacobi_rotation(double app, double aqq, double apq, double &off, double &cs, double &sn)
{
    if (fabs(apq) <= 1e-300 || fabs(apq) <= 1e-17 * sqrt(app * aqq)) return false;
    const double r = fabs(apq) / sqrt(app * aqq);
    off = off < r ? r : off;
    const double zeta = (aqq - app) / (2.0 * apq);
    const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    cs = 1.0 / sqrt(1.0 + t * t);
    sn = cs * t;
    return true;
}

// ---- form A: a lane per (trajectory, sampled step) ------------------------------------------------------------------------
template <int N, int MP>
__global__ void __launch_bounds__(64)
k_svr_lane(int batch, int m, int T, int sampling, int c0, int nc, const double *__restrict__ K, double *__restrict__ stage)
{
    constexpr int dof = N / 2;
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= batch * nc) return;
    const int b = idx / nc, tc = idx - b * nc;
    const int t = (c0 + tc) * sampling;
    const double *Kt = K + ((size_t)b * T + t) * N * m;
    double W[N][MP];
#pragma unroll
    for (int j = 0; j < N; j++)
#pragma unroll
        for (int c = 0; c < MP; c++) W[j][c] = c < m ? Kt[j * m + c] : 0.0;

#pragma unroll 1
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < MP - 1; p++)
#pragma unroll
            for (int q = p + 1; q < MP; q++) {
                if (q >= m) continue;
                double app = 0, aqq = 0, apq = 0;
#pragma unroll
                for (int j = 0; j < N; j++) { app += W[j][p] * W[j][p]; aqq += W[j][q] * W[j][q]; apq += W[j][p] * W[j][q]; }
                double cs, sn;
                if (!jacobi_rotation(app, aqq, apq, off, cs, sn)) continue;
#pragma unroll
                for (int j = 0; j < N; j++) {
                    const double wp = W[j][p], wq = W[j][q];
                    W[j][p] = cs * wp - sn * wq;
                    W[j][q] = sn * wp + cs * wq;
                }
            }
        if (off < 1e-15) break;
    }

    double nrm[MP];
#pragma unroll
    for (int i = 0; i < MP; i++) {
        double s = 0;
#pragma unroll
        for (int j = 0; j < N; j++) s += W[j][i] * W[j][i];
        nrm[i] = sqrt(s);
    }
    // position of column i after std::stable_sort by descending norm: larger norms, and equal norms of lower index, go first
    const int lead = m < 3 ? m : 3;
    double *st = stage + ((size_t)b * nc + tc) * 2 * lead * dof;
#pragma unroll
    for (int i = 0; i < MP; i++) {
        if (i >= m) continue;
        int rank = 0;
#pragma unroll
        for (int c = 0; c < MP; c++)
            if (c < m) rank += (nrm[c] > nrm[i]) || (c < i && nrm[c] == nrm[i]);
        if (rank >= lead) continue;
        const double sg = nrm[i];
#pragma unroll
        for (int j = 0; j < dof; j++) {
            st[(2 * rank) * dof + j] = fabs((sg > 0 ? W[j][i] / sg : 0.0) * sg);
            st[(2 * rank + 1) * dof + j] = fabs((sg > 0 ? W[j + dof][i] / sg : 0.0) * sg);
        }
    }
}

// ---- form B: a wave per (trajectory, sampled step) ------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(64)
k_svr_wave(int dof, int m, int T, int sampling, int c0, int nc, const double *__restrict__ K, double *__restrict__ stage)
{
    extern __shared__ double lds[];
    const int n = 2 * dof, lane = threadIdx.x;
    double *W = lds;                  // [m][n]: column c of W at W + c * n
    double *nrm = lds + (size_t)n * m;
    const int b = blockIdx.x / nc, tc = blockIdx.x - b * nc;
    const int t = (c0 + tc) * sampling;
    const double *Kt = K + ((size_t)b * T + t) * n * m;
    for (int j = lane; j < n; j += 64)
        for (int c = 0; c < m; c++) W[c * n + j] = Kt[j * m + c];

    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0;
        for (int p = 0; p < m - 1; p++)
            for (int q = p + 1; q < m; q++) {
                double app = 0, aqq = 0, apq = 0;
                for (int j = lane; j < n; j += 64) {
                    const double wp = W[p * n + j], wq = W[q * n + j];
                    app += wp * wp; aqq += wq * wq; apq += wp * wq;
                }
                app = wave_sum(app); aqq = wave_sum(aqq); apq = wave_sum(apq);
                double cs, sn;
                if (!jacobi_rotation(app, aqq, apq, off, cs, sn)) continue;
                for (int j = lane; j < n; j += 64) {
                    const double wp = W[p * n + j], wq = W[q * n + j];
                    W[p * n + j] = cs * wp - sn * wq;
                    W[q * n + j] = sn * wp + cs * wq;
                }
            }
        if (off < 1e-15) break;
    }

    for (int i = 0; i < m; i++) {
        double s = 0;
        for (int j = lane; j < n; j += 64) s += W[i * n + j] * W[i * n + j];
        s = wave_sum(s);
        if (lane == 0) nrm[i] = sqrt(s);
    }
    __syncthreads();
    // the stable descending order's first lead columns: the largest norm not yet taken, ties to the lower index
    const int lead = m < 3 ? m : 3;
    double *st = stage + ((size_t)b * nc + tc) * 2 * lead * dof;
    int taken0 = -1, taken1 = -1;
    for (int k = 0; k < lead; k++) {
        int i = -1;
        for (int c = 0; c < m; c++) {
            if (c == taken0 || c == taken1) continue;
            if (i < 0 || nrm[c] > nrm[i]) i = c;
        }
        if (k == 0) taken0 = i; else taken1 = i;
        const double sg = nrm[i];
        for (int r = lane; r < n; r += 64) {
            const int h = r >= dof;
            st[(2 * k + h) * dof + r - h * dof] = fabs((sg > 0 ? W[i * n + r] / sg : 0.0) * sg);
        }
    }
}

// ---- pass 2: one thread per (trajectory, DoF), the host's order of additions ---------------------------------------------
__global__ void __launch_bounds__(64)
k_svr_accumulate(int batch, int dof, int lead, int T, int nc, int first, int last, const double *__restrict__ stage,
                 double *__restrict__ acc)
{
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= batch * dof) return;
    const int b = idx / dof, j = idx - b * dof;
    double s = first ? 0.0 : acc[idx];
    const double *st = stage + (size_t)b * nc * 2 * lead * dof + j;
    for (int tc = 0; tc < nc; tc++)
        for (int k = 0; k < 2 * lead; k++) s += st[((size_t)tc * 2 * lead + k) * dof];
    acc[idx] = last ? s / T : s;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
static int pow2_at_least(int m)
{
    int p = 1;
    while (p < m) p <<= 1;
    return p;
}

bool svr_lane_form(int n, int m)
{
    return n <= 16 && m <= 16 && n * pow2_at_least(m) <= 128;
}

size_t svr_wave_lds_bytes(int n, int m)
{
    return ((size_t)n * m + m) * sizeof(double);
}

typedef void (*SvrLaneKernel)(int, int, int, int, int, int, const double *, double *);

template <int N>
static SvrLaneKernel svr_lane_kernel(int mp)
{
    if (mp == 1) return k_svr_lane<N, 1>;
    if (mp == 2) return k_svr_lane<N, 2>;
    if (mp == 4) return k_svr_lane<N, 4>;
    if constexpr (N * 8 <= 128) if (mp == 8) return k_svr_lane<N, 8>;
    if constexpr (N * 16 <= 128) if (mp == 16) return k_svr_lane<N, 16>;
    return nullptr;
}

static SvrLaneKernel svr_lane_kernel(int n, int m)
{
    const int mp = pow2_at_least(m);
    switch (n) {
    case 2: return svr_lane_kernel<2>(mp);
    case 4: return svr_lane_kernel<4>(mp);
    case 6: return svr_lane_kernel<6>(mp);
    case 8: return svr_lane_kernel<8>(mp);
    case 10: return svr_lane_kernel<10>(mp);
    case 12: return svr_lane_kernel<12>(mp);
    case 14: return svr_lane_kernel<14>(mp);
    case 16: return svr_lane_kernel<16>(mp);
    }
    return nullptr;
}

// the sampled steps of one pass-1 launch: their terms of the whole batch take at most this many bytes of staging
static constexpr size_t kSvrStageBytes = (size_t)256 << 20;

size_t svr_stage_bytes(int batch, int dof, int m, int T, int sampling)
{
    const int lead = m < 3 ? m : 3;
    const size_t per_step = (size_t)batch * 2 * lead * dof * sizeof(double);
    const size_t ns = ((size_t)T + sampling - 1) / sampling;
    size_t nc = kSvrStageBytes / per_step;
    if (nc < 1) nc = 1;
    if (nc > ns) nc = ns;
    return (size_t)batch * dof * sizeof(double) + nc * per_step;
}

bool svr_supported(int n, int m)
{
    return svr_lane_form(n, m) || svr_wave_lds_bytes(n, m) <= 65536;
}

// work: svr_stage_bytes; the sums [batch][dof] at its head (running sums between chunks, divided by T by the last one), the
// staging behind them
hipError_t launch_dof_importance_svd(Ctx *c, int sampling, double *work)
{
    const int B = c->d.batch, dof = c->d.dof, m = c->d.m, T = c->d.T, n = c->n;
    const int lead = m < 3 ? m : 3;
    const size_t per_step = (size_t)B * 2 * lead * dof * sizeof(double);
    const int ns = (int)(((size_t)T + sampling - 1) / sampling);
    const int nc_max = (int)((svr_stage_bytes(B, dof, m, T, sampling) - (size_t)B * dof * sizeof(double)) / per_step);
    double *sums_dev = work, *stage = work + (size_t)B * dof;
    SvrLaneKernel lane = svr_lane_form(n, m) ? svr_lane_kernel(n, m) : nullptr;
    const size_t lds = svr_wave_lds_bytes(n, m);
    for (int c0 = 0; c0 < ns; c0 += nc_max) {
        const int nc = ns - c0 < nc_max ? ns - c0 : nc_max;
        if (lane)
            hipLaunchKernelGGL(lane, dim3((B * nc + 63) / 64), dim3(64), 0, c->stream, B, m, T, sampling, c0, nc, c->K, stage);
        else
            hipLaunchKernelGGL(k_svr_wave, dim3(B * nc), dim3(64), lds, c->stream, dof, m, T, sampling, c0, nc, c->K, stage);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_svr_accumulate, dim3((B * dof + 63) / 64), dim3(64), 0, c->stream, B, dof, lead, T, nc,
                           (int)(c0 == 0), (int)(c0 + nc >= ns), stage, sums_dev);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace kpilqr
