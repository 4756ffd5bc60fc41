// iLQR_GPU_Batch.h -- B independent trajectory optimisations (MPC replans, several initial conditions) driven
// together through ONE kpilqr context with dims.batch = B: the batch analogue of iLQR::Optimise / Iteration
// (src/Optimiser/iLQR.cpp:269-531), with the scalar control flow of the reference kept PER TRAJECTORY:
// lambda schedule and PD retry (:435-442, :636-657), acceptance and the lambda back-off (:490-528),
// convergence (src/Optimiser/Optimiser.cpp:30-37), "skip the derivatives after a rejected step" (:419).
// Every trajectory has its own task / simulator / differentiator objects (the reference's classes are not
// re-entrant); the GPU stages run once per iteration for the whole batch.
#pragma once
#include <memory>
#include <string>
#include <vector>
#include "Differentiator.h"
#include "KeyPointGenerator.h"
#include "ModelTranslator.h"
#include "../../include/kpilqr.h"

class iLQR_GPU_Batch {
public:
    struct Problem {
        std::shared_ptr<ModelTranslator> model_translator;
        std::shared_ptr<PhysicsSimulator> MuJoCo_helper;
        std::shared_ptr<Differentiator> differentiator;
    };
    iLQR_GPU_Batch(std::vector<Problem> problems, int horizon, int device = 0, bool fused = false);
    ~iLQR_GPU_Batch();
    bool ok() const { return ctx != nullptr; }

    // Optimises every trajectory from the state in its simulator's main_data with its initial controls.
    // Returns the optimised controls per trajectory.
    std::vector<std::vector<MatrixXd>> OptimiseAll(const std::vector<std::vector<MatrixXd>> &initial_controls,
                                                   int max_iterations, int min_iterations);

    // per-trajectory results
    std::vector<std::vector<double>> cost_history;
    std::vector<int> num_iterations;
    std::vector<double> lambda;
    std::vector<std::vector<MatrixXd>> K, k;
    // iLQR_SVR's DoF importance (host/SVR.h, DofImportance) of every trajectory on the gains of the last backward pass as the
    // device holds them, either branch, without downloading K: [B][dof]
    std::vector<std::vector<double>> DofImportance(int sampling_k_interval, bool eigen_vector_method);
    kpilqr_ctx *Context() const { return ctx; }
    // line-search statistics of the last iteration, the 8 doubles of the multi-GPU reduction
    // (sum_b J_pred(alpha_1..6), sum_b delta_J, #valid backward passes) -- SURVEY.md section 8e
    double linesearch_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // what crossed the link since construction: FD payload bytes up (whole slabs, or the regenerating trajectories' records alone
    // after a partial regeneration on a fused context), gain bytes down (K, k of the active trajectories with a valid backward
    // pass); and the batch's key-point entries at every linearisation
    size_t payload_bytes_uploaded = 0, gain_bytes_downloaded = 0;
    size_t gain_trajectories_fetched = 0;    // trajectories whose K, k came down, summed over the iterations
    // K comes down as FP32 (kpilqr_download_gains_f32_partial: T*n*m*4 instead of *8 bytes per fetched trajectory) into a pinned float
    // array and is widened into K[b][t], which is exact; k stays FP64.  Off by default: the FP64 gains, bit for bit as before.
    bool gains_f32 = false;
    // ... and the per-iteration inputs: r (and r_x, r_u unless the task's Jacobians are constant) up at every linearisation -- the
    // rows of the regenerating trajectories alone once a complete linearisation is resident -- and U_old up at every iteration, the
    // rows that changed since the last upload alone.  Weights and control limits are not counted.
    size_t residual_bytes_uploaded = 0, nominal_bytes_uploaded = 0;
    // The per-step residual Jacobians cross the link as FP32 (kpilqr_upload_residual_jacobians_f32, or its _partial form where a subset
    // re-linearises): what ResidualDerivativesAll produced is cast -- a plain cast -- into pinned float buffers and the library widens
    // it; r goes up as before.  residual_bytes_uploaded counts the floats as 4 bytes.  Off by default: the FP64 Jacobians, bit for bit
    // as before.  residual_jacobians_f32_on_host: rounded alike, widened on the host and uploaded as FP64 -- the run the FP32 route
    // must reproduce bit for bit.  A task with ConstantResidualJacobians ignores both.
    bool residual_jacobians_f32 = false, residual_jacobians_f32_on_host = false;
    // true: residuals, nominal controls and (on a materialising context) the step records go through the whole-batch calls at every
    // linearisation, as before the partial calls existed -- the A/B of the tests
    bool whole_inputs = false;
    std::vector<int> linearisation_entries;
    // STEP 2's PD retry on the device (kpilqr_set_lambda_retry with lambda_factor, max_lambda and the ABI's largest attempt count): one
    // kpilqr_backward, one kpilqr_download_lambda_retry and one sync per iteration instead of a sync and a whole-batch sweep per
    // retry; lambda[b], valid, lambda_exit and delta_J are rebuilt from (status, lambda_used, attempts) by the code of the host loop.
    // Off by default: the host loop, call for call as before (kpilqr_set_lambda_retry is only ever called with the option on).
    bool device_lambda_retry = false;
    // calls of kpilqr_backward, and sweeps a trajectory repeated at a raised lambda (on either route), since construction
    size_t backward_sweeps = 0, lambda_retries = 0;
    // STEP 2 and STEP 3 over the trajectories that need them (kpilqr_backward_partial, kpilqr_forward_linear_partial): STEP 2 sweeps
    // `active` minus the settled trajectories -- so each host retry sweeps only the trajectories that failed -- and STEP 3 the
    // trajectories with a valid backward pass.  Off by default: the whole-batch calls, call for call as before.
    bool active_sweeps = false;
    // trajectories swept, summed over the calls: batch per call on the default route, the list's length with active_sweeps
    size_t backward_trajectories_swept = 0, forward_trajectories_swept = 0;
    // regularisation / line search constants (include/Optimiser/Optimiser.h:239-242,259,303)
    double max_lambda = 10.0, min_lambda = 0.0001, lambda_factor = 10, epsConverge = 0.02;
    int num_parallel_rollouts = 6;
    // 0: the reference's line search (all alphas rolled out on the trajectory's FD pool, arg-min, accept iff it beats the
    // old cost: iLQR.cpp:463-503); 1: GPU-predicted order, first improving candidate (see iLQR_GPU.h)
    int linesearch_mode = 0;

private:
    struct Traj {
        std::shared_ptr<KeypointGenerator> kpgen;
        std::vector<MatrixXd> U_old, X_old, residuals;
        double old_cost = 0, new_cost = 0, delta_J = 0;
        bool cost_reduced_last_iter = true, done = false, lambda_exit = false;
        std::vector<int> kp_offsets, kp_times;      // per-DoF CSR of the current key-points
    };
    double Rollout(int b, SimData *start, const std::vector<MatrixXd> &controls);
    double ConfirmRollout(int b, int tid, double alpha, std::vector<MatrixXd> &U_out);
    void GenerateDerivatives(const std::vector<int> &who);
    void fatal(const char *what, int rc);

    std::vector<Problem> P;
    std::vector<Traj> S;
    kpilqr_ctx *ctx = nullptr;
    int B, dof, num_ctrl, nr, T, device;
    bool fused_active = false;
    std::vector<double> alphas, w_run, w_term, ctrl_lim;
    FDStaging staging;
    // fused sweeps: the key-point ordered FD payload (kpilqr_upload_fd_kp) of the whole batch in one pinned slab, kept between
    // iterations so that a partial regeneration refills only its trajectories' records while the entry layout stays the same
    char *kp_slab = nullptr;
    size_t kp_slab_bytes = 0;
    char *kp_part = nullptr;                // pinned: the records of a partial regeneration's trajectories, back to back
    size_t kp_part_bytes = 0;
    std::vector<int> kp_slab_offs;          // the batch CSR the slab's records were laid out for (empty: no valid slab)
    bool const_jacobians = false, const_jacobians_resident = false;     // the task's ONE residual Jacobian pair: uploaded once
    bool inputs_resident = false;           // a complete linearisation has happened: every row of r (r_x, r_u) and every record is on the device
    std::vector<char> unom_stale;           // [B] U_old changed since the device's row was uploaded
    std::vector<double> const_rx, const_ru;
    double *host_r = nullptr, *host_rx = nullptr, *host_ru = nullptr, *host_unom = nullptr, *host_K = nullptr, *host_k = nullptr;
    float *host_rx32 = nullptr, *host_ru32 = nullptr;      // residual_jacobians_f32: r_x, r_u as they cross the link, pinned [B][T+1][nr][n | m]; allocated when the option is first used
    float *host_K32 = nullptr;              // gains_f32: K as it crosses the link, pinned [B][T][n][m]; allocated when the option is first used
};

// Moves the key-point records of the trajectories that do NOT regenerate (regen[b] == 0) from their entry offsets in the old batch
// CSR (old_offs [B*dof+1]) to those of the new one (new_offs), in place (src == dst) or into another slab; iLQR_GPU_Batch.cpp.
// Exposed for the unit test of its move order (host_capi: kpilqr_host_relocate_records).
void relocate_records(const char *src, char *dst, size_t stride, int B, int dof, const std::vector<int> &old_offs,
                      const std::vector<int> &new_offs, const std::vector<char> &regen);
