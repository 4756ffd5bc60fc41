// lambda_retry.hip -- kpilqr_set_lambda_retry: the device side of retrying a backward sweep whose PD check failed at a raised lambda
// (the failure branch of iLQR.cpp:435-442 with UpdateLambda, :636-657), without the host.
//
// The sweeps themselves do not change: every backward kernel reads lambda[b] once at its top and writes status[b] once at its end.
// Between two attempts of a call k_lambda_retry looks at the status each trajectory's last sweep left, advances lambda[b] where
// the schedule allows another sweep and writes gate[b]; the next attempt's kernels leave at their first statement where gate[b] is 0,
// so a settled trajectory keeps the bits of its successful sweep and one that gave up keeps its failing status.
//
//   status == 0                        -> settled:  gate 0
//   lambda * factor >  max_lambda      -> gives up: gate 0, lambda stays the lambda of the last sweep
//   otherwise                          -> lambda := lambda * factor, attempts += 1, gate 1
//
// lambda * factor is ONE IEEE multiply (the Makefile builds this file without FMA contraction; there is nothing to contract), the
// comparison is the host loop's: what the caller computes from (status, lambda_used) is what ran here.  One thread per trajectory,
// plain vector loads and stores; a chunk of a streamed iteration runs it on its own slice (the pointers of a view are shifted).
#include "common.h"

namespace kpilqr {

#define KPLR_THREADS 256

// Both kernels take (count, list): thread i works on trajectory list[i], or on trajectory i where list is nullptr (the whole batch).
// In a listed launch (kpilqr_backward_partial; Ctx::sweep_list, d.batch entries) an unlisted trajectory -- whose status may well be
// non-zero from an earlier sweep -- is therefore never armed, and no word of its lambda, attempts or gate is written.  The listed
// sweeps look at the gates of listed trajectories only.

// before the first attempt of a call: every trajectory (of the list) is about to run its first sweep
__global__ void __launch_bounds__(KPLR_THREADS)
k_lambda_retry_begin(int count, const int *__restrict__ list, int *__restrict__ attempts, int *__restrict__ gate)
{
    const int i = blockIdx.x * KPLR_THREADS + threadIdx.x;
    if (i >= count) return;
    const int b = list ? list[i] : i;
    if (attempts) attempts[b] = 1;           // (nullptr: no schedule, the gate alone is armed -- launch_gate_arm)
    gate[b] = 1;
}

// between two attempts.  A trajectory whose gate is already 0 did not run the last attempt: its status is an earlier sweep's and
// it stays out.
__global__ void __launch_bounds__(KPLR_THREADS)
k_lambda_retry(int count, const int *__restrict__ list, double factor, double max_lambda, const int *__restrict__ status,
               double *__restrict__ lambda, int *__restrict__ attempts, int *__restrict__ gate)
{
    const int i = blockIdx.x * KPLR_THREADS + threadIdx.x;
    if (i >= count) return;
    const int b = list ? list[i] : i;
    if (gate[b] == 0) return;
    int again = 0;
    if (status[b] != 0) {
        const double next = lambda[b] * factor;
        if (!(next > max_lambda)) {
            lambda[b] = next;
            attempts[b] += 1;
            again = 1;
        }
    }
    gate[b] = again;
}

static hipError_t launch_begin(Ctx *c, int *attempts)
{
    hipLaunchKernelGGL(k_lambda_retry_begin, dim3((c->d.batch + KPLR_THREADS - 1) / KPLR_THREADS), dim3(KPLR_THREADS), 0, c->stream, c->d.batch,
                       c->sweep_list, attempts, (int *)c->gate);
    return hipGetLastError();
}

hipError_t launch_gate_arm(Ctx *c)
{
    if (c->d.batch <= 0 || !c->sweep_list) return hipSuccess;
    return launch_begin(c, nullptr);
}

hipError_t launch_lambda_retry_begin(Ctx *c)
{
    if (c->d.batch <= 0) return hipSuccess;
    return launch_begin(c, (int *)c->attempts);
}

hipError_t launch_lambda_retry(Ctx *c)
{
    if (c->d.batch <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_lambda_retry, dim3((c->d.batch + KPLR_THREADS - 1) / KPLR_THREADS), dim3(KPLR_THREADS), 0, c->stream, c->d.batch,
                       c->sweep_list, c->retry.factor, c->retry.max_lambda, (const int *)c->status, (double *)c->lambda, (int *)c->attempts,
                       (int *)c->gate);
    return hipGetLastError();
}

}  // namespace kpilqr
