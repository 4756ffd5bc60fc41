// kp_union.hip -- KPILQR_FLAG_UNION_KEYPOINTS: the per-DoF key-point lists of a trajectory re-sampled onto their union.
//
// Per-DoF lists (velocity_change, adaptive_jerk, iterative_error) run the general forms of the one-tile sweeps; lists that are the
// same for every DoF of a trajectory run the faster segment-loop forms.  Giving every DoF the union U_b of its trajectory's
// key-point times makes any set uniform without changing the piecewise-linear function: a column at an inserted time is the
// interpolant k_interpolate (elementwise.hip) writes there.  Three kernels:
//   k_kp_union_count   |U_b| per trajectory (the host reads the counts back, scans them and sizes the union buffers)
//   k_kp_union_build   the union as an ordinary CSR (one copy per DoF list) and kpu_src, the own-list entry behind every union time
//   k_kp_union_expand  kpc -> kpcu, a streaming kernel
// Compiled without FMA contraction, like elementwise.hip: the interpolant has the reference's operation order and roundings.
#include "common.h"

namespace kpilqr {

// A trajectory's key-point times as a bit map in LDS, KPU_BITS steps at a time (longer horizons loop over chunks)
#define KPU_THREADS 256
#define KPU_WORDS 1024
#define KPU_BITS (KPU_WORDS * 32)

// bits [t0, t0 + KPU_BITS) of the map of CSR entries [lo, hi)
__device__ static void kpu_fill(unsigned *map, int t0, int T, int lo, int hi, const int *__restrict__ times)
{
    for (int w = threadIdx.x; w < KPU_WORDS; w += KPU_THREADS) map[w] = 0u;
    __syncthreads();
    for (int e = lo + threadIdx.x; e < hi; e += KPU_THREADS) {
        const int t = times[e];
        if ((unsigned)t < (unsigned)T && t >= t0 && t - t0 < KPU_BITS) atomicOr(&map[(t - t0) >> 5], 1u << ((t - t0) & 31));
    }
    __syncthreads();
}

__global__ void __launch_bounds__(KPU_THREADS)
k_kp_union_count(int dof, int T, const int *__restrict__ offs, const int *__restrict__ times, int *__restrict__ counts)
{
    __shared__ unsigned map[KPU_WORDS];
    __shared__ int total;
    const int b = blockIdx.x;
    const int lo = offs[(size_t)b * dof], hi = offs[(size_t)(b + 1) * dof];      // the trajectory's lists are one contiguous CSR range
    if (threadIdx.x == 0) total = 0;
    for (int t0 = 0; t0 < T; t0 += KPU_BITS) {
        kpu_fill(map, t0, T, lo, hi, times);
        int mine = 0;
        for (int w = threadIdx.x; w < KPU_WORDS; w += KPU_THREADS) mine += __popc(map[w]);
        if (mine) atomicAdd(&total, mine);
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[b] = total;
}

// first [batch+1]: union times before trajectory b (the host's scan of the counts).  A thread owns four consecutive words of the
// map: a block scan of the threads' popcounts ranks its bits, and every set bit is written to the union list of each DoF with
// its kpu_src -- upper_bound in the DoF's own list, a few steps over a list that is in cache (built once per key-point change).
__global__ void __launch_bounds__(KPU_THREADS)
k_kp_union_build(int batch, int dof, int T, const int *__restrict__ offs, const int *__restrict__ times, const int *__restrict__ first,
                 int *__restrict__ u_offs, int *__restrict__ u_times, int *__restrict__ u_src)
{
    __shared__ unsigned map[KPU_WORDS];
    __shared__ int scan[KPU_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lo = offs[(size_t)b * dof], hi = offs[(size_t)(b + 1) * dof];
    const int f0 = first[b], cnt = first[b + 1] - f0;
    const size_t base = (size_t)dof * f0;                // first union entry of the trajectory
    if (tid < dof) u_offs[(size_t)b * dof + tid] = (int)(base + (size_t)tid * cnt);
    if (b == batch - 1 && tid == 0) u_offs[(size_t)batch * dof] = dof * first[batch];
    int before = 0;                                      // union times in the chunks already done
    for (int t0 = 0; t0 < T; t0 += KPU_BITS) {
        kpu_fill(map, t0, T, lo, hi, times);
        constexpr int per = KPU_WORDS / KPU_THREADS;
        int mine = 0;
        for (int i = 0; i < per; i++) mine += __popc(map[tid * per + i]);
        scan[tid] = mine;
        __syncthreads();
        for (int s = 1; s < KPU_THREADS; s <<= 1) {      // inclusive scan
            const int add = tid >= s ? scan[tid - s] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        int rank = before + scan[tid] - mine;
        before += scan[KPU_THREADS - 1];
        for (int i = 0; i < per; i++) {
            unsigned bits = map[tid * per + i];
            while (bits) {
                const int t = t0 + (tid * per + i) * 32 + (__ffs(bits) - 1);
                bits &= bits - 1;
                if (rank < cnt) {
                    for (int d = 0; d < dof; d++) {
                        const int lo_d = offs[(size_t)b * dof + d], hi_d = offs[(size_t)b * dof + d + 1];
                        int l = lo_d, h = hi_d;          // upper_bound(t) - 1: the key-point at or before t
                        while (l < h) {
                            const int mid = (l + h) >> 1;
                            if (times[mid] <= t) l = mid + 1; else h = mid;
                        }
                        // (canonical lists start at 0: p >= lo_d; the clamp keeps a list that does not from indexing outside itself)
                        const int p = l - 1 < lo_d ? lo_d : l - 1;
                        const size_t eu = base + (size_t)d * cnt + rank;
                        u_times[eu] = t;
                        u_src[eu] = (times[p] == t || p + 1 >= hi_d) ? ~p : p;
                    }
                }
                rank++;
            }
        }
        __syncthreads();                                 // (the next chunk clears the map)
    }
}

// kpc -> kpcu.  A thread owns two consecutive rows of one (union entry, kind): 3n contiguous doubles per entry in and out, 16-byte
// accesses.  kpu_src is the only indirection; an own key-point copies its column, an inserted time u between the DoF's key-points
// s < u < e gets start + (u - s) * ((end - start) / (e - s)) in exactly k_interpolate's order (IEEE quotient, no contraction):
// bit for bit what kpilqr_interpolate writes at that step.
__global__ void __launch_bounds__(256)
k_kp_union_expand(int n, long long npairs_total, unsigned long long magic, const int *__restrict__ u_times, const int *__restrict__ u_src,
                  const int *__restrict__ times, const double2 *__restrict__ kpc, double2 *__restrict__ kpcu)
{
    const int pe = 3 * (n >> 1);                     // pairs per entry
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < npairs_total; w += stride) {
        const long long eu = magic ? (long long)__umul64hi((unsigned long long)w, magic) : w;      // w / pe
        const int p = (int)(w - eu * pe);
        const int src = u_src[eu];
        const bool own = src < 0;
        const long long ent = own ? ~src : src;
        double2 v = kpc[ent * pe + p];
        if (!own) {
            const int cs = times[ent], ce = times[ent + 1], t = u_times[eu];
            const double2 ve = kpc[(ent + 1) * pe + p];
            double2 add;
            add.x = (ve.x - v.x) / (double)(ce - cs);
            add.y = (ve.y - v.y) / (double)(ce - cs);
            v.x = v.x + ((double)(t - cs) * add.x);
            v.y = v.y + ((double)(t - cs) * add.y);
        }
        kpcu[w] = v;
    }
}

hipError_t launch_kp_union_count(Ctx *c)
{
    hipLaunchKernelGGL(k_kp_union_count, dim3(c->d.batch), dim3(KPU_THREADS), 0, c->stream, c->d.dof, c->d.T, c->kp_offsets, c->kp_times,
                       c->kpu_traj_first);
    return hipGetLastError();
}

hipError_t launch_kp_union_build(Ctx *c)
{
    hipLaunchKernelGGL(k_kp_union_build, dim3(c->d.batch), dim3(KPU_THREADS), 0, c->stream, c->d.batch, c->d.dof, c->d.T, c->kp_offsets,
                       c->kp_times, c->kpu_traj_first, c->kpu_offsets, c->kpu_times, c->kpu_src);
    return hipGetLastError();
}

hipError_t launch_kp_union_expand(Ctx *c)
{
    const long long entries = (long long)c->d.dof * c->kpu_total;
    if (entries == 0) return hipSuccess;
    const int pe = 3 * (c->n >> 1);
    const long long npairs = entries * pe;
    const unsigned long long magic = pe > 1 ? ~0ULL / (unsigned)pe + 1ULL : 0ULL;
    const long long want = (npairs + 256LL * 4 - 1) / (256LL * 4);
    const long long cap = (long long)(c->n_simd / 4) * 128;
    const int blocks = (int)(want < cap ? (want < 1 ? 1 : want) : cap);
    hipLaunchKernelGGL(k_kp_union_expand, dim3(blocks), dim3(256), 0, c->stream, c->n, npairs, magic, c->kpu_times, c->kpu_src, c->kp_times,
                       (const double2 *)(double *)c->kpc, (double2 *)(double *)c->kpcu);
    return hipGetLastError();
}

}  // namespace kpilqr
