/*
 * kpilqr.h -- C ABI of libkpilqr.so: the MI355X (gfx950) engine for the numerical hot path of
 * keypoint-interpolated iLQR.  It is the drop-in boundary for the reference DMackRus/TrajOptKP:
 * a C++ `Optimiser` subclass (see INTEGRATION.md, and trajoptkp_amd/host/ for the one shipped
 * here) forwards STEP 1b/1c/2/3 of iLQR::Iteration (src/Optimiser/iLQR.cpp:412-531) to these
 * entry points; MuJoCo and the ModelTranslator stay on the host.
 *
 * The reference has no FFI of its own (its plugin surface is three C++ classes wired with
 * shared_ptr in src/main.cpp:39-47,114-147); each entry point below names the reference
 * function it replaces.  Paths are relative to the reference repository root.
 *
 * Conventions
 *  - plain C, no torch / Eigen / HIP types in any signature; `stream` is a hipStream_t passed as
 *    void* (NULL = the library creates its own non-blocking stream).
 *  - all floating point data is FP64.  Host-side matrices use the reference's Eigen layout:
 *    COLUMN-MAJOR per matrix, one matrix per time-step, time-major then batch-major:
 *    A[b][t] at A + ((b*T + t)*n*n), element (r,c) at r + c*n.   n = 2*dof, m = num_ctrl.
 *  - device buffers are owned by the context (internal layout: DESIGN.md section 3).
 *  - every call returns int: 0 = ok, <0 = error (kpilqr_strerror), >0 = numerical status.
 *    Calls that launch kernels are asynchronous on the context's stream; host output buffers
 *    are valid after kpilqr_sync().  One context per (GPU, host thread); not re-entrant.
 *  - the library FAILS LOUDLY (negative code) when no HIP device is present: there is no CPU
 *    fallback inside it.
 */
#ifndef KPILQR_H
#define KPILQR_H

#include <stddef.h>

/* ---- Diagnostic environment switches ------------------------------------------------------------
 * NOT part of the ABI: a caller never needs them, the defaults are what the library has measured to be fastest, and every
 * form gives the same results (to the tolerances of the tests).  They exist so that tests can reach a kernel form the batch
 * size would not select, and for same-box A/B timing; kpilqr_last_launch reports what actually ran.  All are read ONCE, in
 * kpilqr_create (changing the environment afterwards has no effect on an existing context); unset or empty = default.
 *
 *   KPILQR_FUSED_WAVES      backward sweep of a FUSED context: 1 one wavefront per trajectory | 5 consumer / helper pair.
 *                           Default: 5 while 2 x batch <= #SIMDs, else 1.  (Any other value = default.)
 *   KPILQR_FUSED_FWD_WAVES  forward sweep of a FUSED context: 1 one wave | 3 state / cost / staging triple | 4 state /
 *                           cost pair for uniform key-point sets with 3 or 1 behind it for per-DoF lists.
 *                           Default: 4 while 2 x batch <= #SIMDs, else 1.  (Any other value = default.)
 *   KPILQR_FUSED_RAW        0: a key-point ordered payload is differenced by k_fd_kp_difference in front of the backward
 *                           sweep instead of inside it (default: inside, for uniform key-point sets).
 *   KPILQR_FUSED_UNI        0: the general (per-DoF list) forms of the one-wave sweeps also for uniform key-point sets.
 *   KPILQR_FD_INTERP        0: a context with step records differences and interpolates a key-point ordered or column payload
 *                           in the separate passes (k_fd_kp_difference, k_kpc_to_records, k_interpolate) instead of in one
 *                           (k_fd_kp_interpolate); same bits either way.  kpilqr_last_launch(ctx, 2) says which ran.
 *   KPILQR_ROLE_SHIFT       wave pairs: block-index bit from which the two roles swap wave slots (default 9; 0 = every
 *                           other block).  Placement probe; no effect on results.
 *   KPILQR_TILED_UW         tiled backward sweep (n + 2 > 16): 1 u-wave form | 0 column-wave form (default by tile count).
 *   KPILQR_TILED_A6         tiled sweeps: 1 / 0 cost derivatives (a6) inside the sweep (default: inside at four tiles from
 *                           ~100 trajectories).
 *   KPILQR_TILED_FSC        two-tile forward sweep: 1 / 0 state / cost wave groups (default: on while 2 NT B <= #SIMDs; never past 0x7fffff00 B of records a trajectory).
 *   KPILQR_TILED_NT_MIN     run the tiled kernels with at least this many tiles (test coverage of a tile count on a
 *                           small state).
 *   KPILQR_PIPE_COPY        kpilqr_iterate_streamed: bit 0 uploads / bit 1 downloads by copy kernels instead of SDMA
 *                           (default 2).  Bit 1 does not reach the K32 and gain_traj downloads of kpilqr_iterate_streamed2:
 *                           they always leave through the gather kernel (a converted or gathered download through SDMA would
 *                           need the staging buffer that call avoids).
 * The host-side thread count of the FD pool is a constructor argument of the host classes, not an environment switch. */

#ifdef __cplusplus
extern "C" {
#endif

#define KPILQR_VERSION 410   /* 0.4.1: same entry points and structs as 400; callers should check kpilqr_version() / 100 == 4 */

typedef struct kpilqr_ctx kpilqr_ctx;

typedef struct {
    int dof;       /* position DoFs of the optimiser's state vector (stateVectorList::dof)      */
    int m;         /* num_ctrl                                                                  */
    int T;         /* horizon_length                                                            */
    int nr;        /* residual_list.size()                                                      */
    int batch;     /* independent trajectories resident in this context                         */
    int n_alpha;   /* num_parallel_rollouts, include/Optimiser/Optimiser.h:259 (6)              */
    int device;    /* HIP device ordinal                                                        */
    int flags;     /* KPILQR_FLAG_*                                                             */
} kpilqr_dims;

#define KPILQR_FLAG_GENERIC_KERNELS 1   /* force the dimension-generic LDS kernels (no MFMA path) */
#define KPILQR_FLAG_TILED_KERNELS   2   /* prefer the LDS-tiled MFMA kernels even when one tile would do */
#define KPILQR_FLAG_FUSED           4   /* n+2 <= 16 only: kpilqr_backward / kpilqr_forward_linear / kpilqr_iterate
                                           evaluate the interpolation (a4) and the cost derivatives (a6) inside the
                                           sweeps, from the differenced key-point columns (a compact column store; with
                                           the key-point ordered payload of kpilqr_upload_fd_kp and one wavefront per
                                           trajectory the backward sweep even does the differencing itself) and the
                                           uploaded residuals; A, B, l_* are then NOT materialised and the context holds
                                           NO step records (kpilqr_interpolate / kpilqr_cost_derivs / get_AB allocate and
                                           fill them on request; the set_AB / set_cost_derivs hooks do not feed the fused
                                           sweeps).  Needs canonical key-points: per DoF strictly increasing, first 0, last T-1.
                                           Faster at every batch size (Panda, T=3000: 170 vs 142 iterations/s for one
                                           trajectory, 102k vs 68k at batch 1024).  On a tiled shape (n+2 > 16) the
                                           library may form only the cost derivatives inside the sweeps (variant
                                           "mfma_f64_tiled_a6": four-tile states from ~100 trajectories up); A and B
                                           are then still materialised and kpilqr_iterate skips kpilqr_cost_derivs. */
#define KPILQR_FLAG_UNION_KEYPOINTS 8   /* Opt-in, together with KPILQR_FLAG_FUSED on a one-tile shape (n+2 <= 16); ignored
                                           otherwise, the way FUSED is on an unsupported shape.  Per-DoF key-point lists
                                           (velocity_change, adaptive_jerk, iterative_error) run the general forms of the fused
                                           sweeps; with this flag kpilqr_backward / kpilqr_forward_linear / kpilqr_iterate give
                                           every DoF of a trajectory the UNION of that trajectory's key-point times -- a column
                                           at an inserted time is the interpolant kpilqr_interpolate writes at that step, bit
                                           for bit -- so the lists are uniform and the segment-loop forms of the sweeps run on a
                                           union column store (kpilqr_last_launch: "...:union").  The piecewise-linear A(t), B(t)
                                           are the same functions; re-interpolating between union times instead of between a
                                           DoF's own key-points changes roundings at the 1e-16 level (K, k, delta_J, predicted
                                           costs within ~4e-15 relative of the per-DoF forms; the tests hold both to 1e-9 of the
                                           oracle).  That difference is why kpilqr_get_keypoints, kpilqr_interpolate,
                                           kpilqr_fd_interpolate and kpilqr_get_AB keep working on the CALLER's lists and keep
                                           the reference's bits.  Cost: ONE wait for the stream per key-point change (the
                                           per-trajectory union sizes, 4 * batch bytes, are read back to size the store), the
                                           differencing and expansion kernels in front of the sweeps, and the union store:
                                           dof * sum_b |U_b| entries of 3n doubles beside the column store's sum of the list
                                           lengths (about 6x at lists on 7 % of the steps whose union covers 41 %).  Lists
                                           the host knows to be uniform (kpilqr_set_keypoints saw equal lists, set_interval)
                                           allocate and launch nothing of this.  kpilqr_backward_stats and
                                           kpilqr_iterate_streamed ignore the flag.  The speed of the route rests on the byte
                                           model of DESIGN.md section 9, not on a measurement (profiles/union_keypoints.txt
                                           holds the procedure): the flag is off by default.  KPILQR_VERSION is unchanged: detect the
                                           feature by the symbols kpilqr_get_union_keypoints / kpilqr_get_union_columns. */
#define KPILQR_FLAG_EMBED_SHAPE    16   /* Embedded shapes.  Opt-in, together with KPILQR_FLAG_FUSED; ignored, the way FUSED is on an
                                           unsupported shape, when the shape has sweep kernels of its own ((dof, m) = (7,7), (2,1),
                                           (6,3), (5,3)), when GENERIC or TILED kernels are forced, and when no carrier exists.
                                           Contract.  A one-tile model of any other shape -- a 6-DoF arm (6,6), a 3-link (3,3), a
                                           pendulum (1,1) ... -- runs the fused sweeps of its CARRIER: the compiled shape (dof', m')
                                           with the smallest n' = 2 dof', then the smallest m', such that dof <= dof' and m <= m';
                                           it needs m <= dof, 1 <= nr <= 16, n_alpha <= 16 and a payload of the carrier's shape within
                                           the sweeps' 2^30-byte offsets.  The caller's problem is zero-embedded at this boundary by
                                           streaming kernels (embed.hip): state row i goes to row i (i < dof) or i + dof' - dof
                                           (velocities), controls are a prefix; padded states get zero A columns and rows, zero B rows
                                           and zero r_x columns, padded controls zero B columns.  The padded block of V then stays
                                           exactly 0, the padded block of Q_uu + lambda I is lambda I, the padded rows of K and k are
                                           exactly 0 and the real block sees only additions of exact zeros: K, k, delta_J, status and the
                                           predicted costs are those of the caller's own problem (the CPU oracle gives identical bits
                                           for both; the device results are bit for bit those of a context created at the carrier's
                                           shape and fed the zero-padded problem).  Every array of the calls in scope keeps the
                                           CALLER's shape: kpilqr_set_keypoints (batch * dof lists, canonical as ever; the padded DoFs
                                           get copies of the trajectory's list 0, so uniform lists stay uniform), kpilqr_fd_kp_layout
                                           (the caller's n) + kpilqr_upload_fd_kp and kpilqr_upload_kp_columns (`entries` = the
                                           caller's kp_offsets[batch*dof]), kpilqr_upload_residuals,
                                           kpilqr_upload_residual_jacobians_const (padded on the host: ":rxc" / ":ru0" as on the
                                           carrier), kpilqr_upload_nominal (padded control limits: (-1, 1)), kpilqr_backward,
                                           kpilqr_forward_linear, kpilqr_iterate, kpilqr_download_gains, kpilqr_download_gains_f32, kpilqr_set_lambda_retry /
                                           kpilqr_download_lambda_retry, kpilqr_trajectory_cost, kpilqr_allreduce_linesearch, kpilqr_comm_*,
                                           kpilqr_sync, kpilqr_host_alloc / kpilqr_host_free, kpilqr_strerror, kpilqr_device_ptr of the shape-free
                                           buffers (residuals, cost_pred, delta_J, status).  kpilqr_get_dims reports the caller's dims,
                                           kpilqr_get_carrier_dims the carrier's; the variant strings are "mfma_f64_t1_fused" and
                                           kpilqr_last_launch(ctx, 0 | 1) ends in ":emb<n'>x<m'>", e.g. ":emb14x7".
                                           The lambda rule.  With padded controls (m' > m) a lambda[b] <= 0 or NaN that the host can see
                                           is refused by kpilqr_backward and kpilqr_iterate with KPILQR_ERR_ARG before anything is
                                           enqueued: the padded block of Q_uu + lambda I is lambda I, so lambda = 0 would fail the first
                                           PD check of every trajectory.  lambda = NULL (the resident lambdas) is accepted; with
                                           m' == m (e.g. (1,1) in (2,1)) lambda = 0 is legal.
                                           Costs.  The sweeps do the carrier's work ((14,7)'s for a (6,6) arm); every by-shape upload is
                                           ONE hipMemcpyAsync into a staging buffer the context owns (as large as the largest such
                                           transfer, kept) and ONE launch; the gains leave through ONE gathering launch per array and
                                           ONE copy in the caller's compact layout; device buffers have the carrier's size.  Measured
                                           once (profiles/embedded_shapes.txt; T = 3000, uniform lists, constant Jacobian): kpilqr_iterate
                                           at (6,6) 4.17 against 7.52 ms of the tiled kernels at B = 64 and 5.19 against 24.03 ms at
                                           B = 1024, at (3,2) 3.47 against 6.22 and 4.12 against 18.07 ms; the gain download 0.44 .. 0.77
                                           of the plain download of the carrier's arrays; the embedding launches add 2.5 .. 6.9 % to
                                           the payload upload and the gain download.  It won at every size measured; per-DoF lists and
                                           shapes much smaller than their carrier have not been timed: the flag is off by default.
                                           Out of scope on an embedded context -- each of these returns KPILQR_ERR_STATE, names itself,
                                           says "not on an embedded context", enqueues nothing and leaves the context as it was:
                                           kpilqr_resize; kpilqr_update_keypoints, kpilqr_upload_fd_kp_partial,
                                           kpilqr_upload_kp_columns_partial, kpilqr_upload_kp_columns_f32,
                                           kpilqr_upload_kp_columns_f32_partial, kpilqr_download_gains_partial,
                                           kpilqr_download_gains_f32_partial, kpilqr_upload_residuals_partial,
                                           kpilqr_upload_residual_jacobians_f32, kpilqr_upload_residual_jacobians_f32_partial,
                                           kpilqr_upload_nominal_partial, kpilqr_fd_interpolate_partial, kpilqr_cost_derivs_partial,
                                           kpilqr_backward_partial, kpilqr_forward_linear_partial, kpilqr_iterate_partial;
                                           kpilqr_iterate_streamed, kpilqr_iterate_streamed2, kpilqr_iterate_streamed3,
                                           kpilqr_iterate_streamed4, kpilqr_iterate_streamed5, kpilqr_iterate_streamed6;
                                           kpilqr_upload_fd, kpilqr_fd_slab_layout,
                                           kpilqr_upload_fd_slab; kpilqr_upload_states, kpilqr_upload_states_partial,
                                           kpilqr_generate_keypoints, kpilqr_generate_keypoints_partial, kpilqr_keypoint_error_test,
                                           kpilqr_get_keypoints, kpilqr_get_keypoints_partial; kpilqr_fd_difference, kpilqr_interpolate,
                                           kpilqr_fd_interpolate, kpilqr_cost_derivs, kpilqr_set_AB, kpilqr_get_AB,
                                           kpilqr_set_cost_derivs, kpilqr_get_cost_derivs; kpilqr_filter_dynamics, kpilqr_dof_importance,
                                           kpilqr_dof_importance_svd, kpilqr_backward_stats; kpilqr_get_union_keypoints,
                                           kpilqr_get_union_columns (KPILQR_FLAG_UNION_KEYPOINTS is ignored); kpilqr_device_ptr of a
                                           shape-dependent buffer.  No environment switch.  KPILQR_VERSION is unchanged: detect the
                                           feature by the symbol kpilqr_get_carrier_dims. */

enum {
    KPILQR_OK = 0,
    KPILQR_ERR_ARG = -1,       /* bad argument / size mismatch (reference: setters return false) */
    KPILQR_ERR_NO_DEVICE = -2, /* no HIP device / runtime failure at create                      */
    KPILQR_ERR_HIP = -3,       /* a HIP call failed; see kpilqr_strerror                          */
    KPILQR_ERR_ALLOC = -4,
    KPILQR_ERR_STATE = -5      /* call order violated (e.g. interpolate before set_keypoints)     */
};

/* which device buffer kpilqr_device_ptr returns */
enum {
    KPILQR_BUF_STEP_RECORDS = 0, /* [batch][T][rec] : A|B|l_xx|l_x|l_uu|l_u per step; a FUSED
                                    context has none until this (or a materialising call) asks for them */
    KPILQR_BUF_K = 1,            /* [batch][T][n][m]  (column-major m x n, as Eigen)             */
    KPILQR_BUF_k = 2,            /* [batch][T][m]                                                */
    KPILQR_BUF_RESIDUALS = 3,    /* [batch][T+1][nr]                                             */
    KPILQR_BUF_R_X = 4,          /* [batch][T+1][nr][n]                                          */
    KPILQR_BUF_R_U = 5,          /* [batch][T+1][nr][m]                                          */
    KPILQR_BUF_U_NOM = 6,        /* [batch][T][m]                                                */
    KPILQR_BUF_FD_XPLUS = 7,     /* [jobs][n]                                                    */
    KPILQR_BUF_FD_XMINUS = 8,    /* [jobs][n]                                                    */
    KPILQR_BUF_COST_PRED = 9,    /* [batch][n_alpha]                                             */
    KPILQR_BUF_DELTA_J = 10,     /* [batch]                                                      */
    KPILQR_BUF_STATUS = 11       /* [batch] int32                                                */
};

/* ---- lifetime --------------------------------------------------------------------------
 * Replaces iLQR::iLQR / iLQR::Resize allocation of A,B,l_*,K,k (src/Optimiser/iLQR.cpp:4-200). */
int  kpilqr_create(const kpilqr_dims *dims, void *stream, kpilqr_ctx **out);
void kpilqr_destroy(kpilqr_ctx *ctx);
int  kpilqr_version(void);
const char *kpilqr_strerror(kpilqr_ctx *ctx);       /* last error text of this context (or global) */
int  kpilqr_get_dims(kpilqr_ctx *ctx, kpilqr_dims *out);   /* the caller's dims, also on an embedded context */
/* KPILQR_FLAG_EMBED_SHAPE: the dims of the carrier shape the sweeps of an embedded context run at (dof', m'; everything else as
 * kpilqr_get_dims).  KPILQR_ERR_STATE on a context that is not embedded (flag not set, or ignored for its shape). */
int  kpilqr_get_carrier_dims(kpilqr_ctx *ctx, kpilqr_dims *out);
/* iLQR_SVR::Resize (src/Optimiser/iLQR_SVR.cpp:38-193): the state-vector reduction changes dof (and possibly num_ctrl,
 * horizon) between optimisations.  Re-sizes the context IN PLACE: device allocations are kept and only grown when the new
 * sizes do not fit; kernel families are re-selected; everything uploaded before is forgotten.  Synchronous. */
int  kpilqr_resize(kpilqr_ctx *ctx, int new_dof, int new_num_ctrl, int new_horizon);

/* Pinned host staging memory (the "one pinned hipMemcpyAsync" of the design).  kpilqr_host_free accepts ctx = NULL: an
 * allocation may be released after the context it was made through has been destroyed (bindings whose arrays outlive the
 * engine object); it must not be in use by a transfer still in flight. */
int  kpilqr_host_alloc(kpilqr_ctx *ctx, size_t bytes, void **pinned);
int  kpilqr_host_free(kpilqr_ctx *ctx, void *pinned);

int  kpilqr_sync(kpilqr_ctx *ctx);
int  kpilqr_device_ptr(kpilqr_ctx *ctx, int which, void **dptr, size_t *bytes);

/* ---- STEP 1b: dynamics derivatives -------------------------------------------------------
 * Key-points per DoF: kp_times[kp_offsets[b*dof+i] .. kp_offsets[b*dof+i+1]) = sorted time
 * indices at which DoF i of trajectory b is finite-differenced (the transpose of the reference's
 * std::vector<std::vector<int>> keypoints, include/KeyPointGenerator.h:85-100).  */
int  kpilqr_set_keypoints(kpilqr_ctx *ctx, const int *kp_offsets, const int *kp_times);

/* ---- partial re-linearisation: new lists, and a new payload, for SOME trajectories -------------------------------------------
 * Only trajectories whose last step was accepted regenerate their derivatives (src/Optimiser/iLQR.cpp:419), but a payload laid out
 * by CSR entry has to follow the lists, and new lists of one trajectory shift the entry offsets of every later one.  These calls
 * keep what is unchanged on the device: the records of the trajectories that are NOT listed are moved to their new entry offsets
 * there (an HBM-rate copy, kp_partial.hip), and only the listed trajectories' records cross the link.
 * `traj` [count] is strictly increasing and within [0, batch) in all four calls; anything else is KPILQR_ERR_ARG.  All four first
 * order themselves behind a kpilqr_iterate_streamed still in flight.  KPILQR_VERSION is unchanged: detect them by their symbols.
 *
 * kpilqr_update_keypoints replaces the per-DoF lists of the listed trajectories -- kp_offsets [count*dof + 1] starts at 0 and
 * indexes kp_times, trajectories in `traj` order, checked exactly as kpilqr_set_keypoints checks (range, monotone offsets) -- and
 * keeps everybody else's.  It leaves the context exactly as kpilqr_set_keypoints with the merged lists would (device CSR, segment
 * maps, canonical / uniform flags, kpilqr_get_keypoints, the union lists invalid), with one exception: a resident payload laid out
 * by entry SURVIVES -- the slab of kpilqr_upload_fd_kp, or the columns of kpilqr_upload_kp_columns.  The listed trajectories'
 * entry ranges are then PENDING: until the matching partial upload below arrives, every call that would read the payload returns
 * KPILQR_ERR_STATE and names what is missing (kpilqr_backward, kpilqr_backward_stats, kpilqr_iterate, kpilqr_iterate_streamed
 * without a new payload, kpilqr_fd_difference, kpilqr_interpolate, kpilqr_fd_interpolate, kpilqr_get_AB, kpilqr_get_union_columns
 * and whatever else would difference it), and so does another kpilqr_update_keypoints.  A whole new payload (kpilqr_upload_fd_kp,
 * kpilqr_upload_kp_columns, kpilqr_upload_fd / _slab, a payload of kpilqr_iterate_streamed) or new lists for everybody
 * (kpilqr_set_keypoints, kpilqr_generate_keypoints) clear the pending state at any time.  With a job-list payload, or with none,
 * there is nothing to carry: the call behaves exactly like kpilqr_set_keypoints on the merged lists.  count = 0 is a no-op:
 * nothing becomes invalid.  A rejected call leaves the context as it was.
 * Cost.  (1) The context keeps a host mirror of all offsets, 4 * (batch*dof + 1) bytes, filled by kpilqr_set_keypoints; after
 * kpilqr_generate_keypoints it is read back on the first update, which WAITS for the stream.  The call also waits for its own
 * copies (the merged offsets are staged in memory it owns), i.e. for the relocation.  (2) The relocation is never in place -- ranges
 * move both ways -- so the context gets SECOND buffers for the by-entry payload and the list times, reserved the first time an update
 * has something to carry and swapped with the live ones after the copy: the by-entry payload allocation is DOUBLED once this
 * route has been used (5.9 GB more at Panda reaching, T = 3000, batch 1024, velocity_change lists).  An update whose new total
 * exceeds the capacity grows the second buffer first and copies before anything is freed: the kept records are never lost.
 * Not through a view of kpilqr_iterate_streamed's chunks (never allocates).
 *
 * kpilqr_upload_fd_kp_partial / kpilqr_upload_kp_columns_partial complete the payload: the slab (records of kpilqr_fd_kp_layout)
 * or column array ([entries][3][n]) holds the records of the listed trajectories back to back in `traj` order.  `traj` must be
 * exactly the pending set and `entries` the sum of their entry counts (else KPILQR_ERR_ARG); eps must match the resident
 * payload's bit for bit (else KPILQR_ERR_ARG: a context has one eps); the payload kind must be the resident kind (else
 * KPILQR_ERR_STATE).  One hipMemcpyAsync per run of adjacent listed trajectories, straight into place, no kernel; pinned / pageable
 * behaviour as kpilqr_upload_fd_kp.  Afterwards the payload is complete and everything derived from it is stale, as after a whole
 * upload (the column store, slope store, union store and step records are re-derived).
 *
 * kpilqr_download_gains_partial writes K [count][T][n][m] and k [count][T][m] of the listed trajectories, compact, in the
 * per-trajectory layout of kpilqr_download_gains: one copy per array and run of adjacent trajectories, asynchronous; either
 * pointer may be NULL.
 *
 * Out of scope: job-list payloads are not carried; the chunks of kpilqr_iterate_streamed are unchanged; nothing derived from the
 * payload stays valid across an update; and kpilqr_generate_keypoints places key-points for the whole batch only.  (Residuals,
 * nominal controls and step records of a subset: the calls further down, "partial re-linearisation, the rest".)
 * (since: kpilqr_generate_keypoints_partial places key-points for a listed subset -- "Key-point placement for a subset".) */
int  kpilqr_update_keypoints(kpilqr_ctx *ctx, int count, const int *traj,
                             const int *kp_offsets /* [count*dof + 1], starts at 0 */, const int *kp_times);
int  kpilqr_upload_fd_kp_partial(kpilqr_ctx *ctx, int count, const int *traj,
                                 const void *slab, int entries, double eps);
int  kpilqr_upload_kp_columns_partial(kpilqr_ctx *ctx, int count, const int *traj,
                                      const double *columns, int entries);
int  kpilqr_download_gains_partial(kpilqr_ctx *ctx, int count, const int *traj,
                                   double *K /* [count][T][n][m] */, double *k /* [count][T][m] */);

/* ---- partial re-linearisation, the rest: residuals, nominal controls and step records of SOME trajectories -------------------
 * What else a linearisation of a subset moves and recomputes.  All four calls take (count, traj) with the contract of
 * kpilqr_update_keypoints: `traj` [count] strictly increasing and within [0, batch), else KPILQR_ERR_ARG and nothing is enqueued or
 * changed; count = 0 is a no-op returning KPILQR_OK; a NULL context is KPILQR_ERR_ARG; not through a view of
 * kpilqr_iterate_streamed's chunks (KPILQR_ERR_STATE).  Host arrays are COMPACT: the listed trajectories' rows back to back in `traj`
 * order.  Copies go out as one hipMemcpyAsync per array and run of adjacent trajectories, straight to their place (as
 * kpilqr_download_gains_partial): no staging buffer, no scatter kernel.  KPILQR_VERSION is unchanged: detect them by their symbols.
 *
 * kpilqr_upload_residuals_partial: r [count][T+1][nr], r_x [count][T+1][nr][n], r_u [count][T+1][nr][m]; NULL = not sent.  Weights
 * stay with kpilqr_upload_residuals.  Rows of a subset never change the form the sweeps run in, so each of these is refused with
 * KPILQR_ERR_STATE, changes nothing, and names the whole-batch call to make first:
 *   r_x  in constant-Jacobian mode (kpilqr_upload_residual_jacobians_const), or before a whole r_x has been uploaded -- every
 *        other row of the buffer has to mean something;
 *   r_u  before a whole r_u upload or broadcast: a context that runs the r_u-free sweeps (":ru0") is not flipped by a few rows.
 * r has no precondition.  Nothing else changes state: payload, key-points, pending ranges and kpilqr_last_launch are untouched.
 * The odd-residual-count rule of kpilqr_upload_residuals ("all T+1 rows finite") applies to the rows sent.
 * kpilqr_upload_nominal_partial: u_nom [count][T][m] (NULL = not sent); control limits stay with kpilqr_upload_nominal.
 *
 * kpilqr_fd_interpolate_partial / kpilqr_cost_derivs_partial are kpilqr_fd_interpolate / kpilqr_cost_derivs for the listed
 * trajectories only: in their records the results are bit for bit what the whole-batch call writes there, and no byte of any
 * other trajectory's records is written.  The caller's contract: the other trajectories' records hold a complete linearisation from
 * an earlier whole or partial call, and their lists, payload, residuals and weights have not changed since.  ONE launch per stage
 * for the whole list, however scattered it is (the kernels read the trajectory of a block row from a device copy of the list,
 * batch ints held by the context, filled by one hipMemcpyAsync; the call waits for the stream only when `traj` is pageable, as
 * kpilqr_set_keypoints does).  With a job-list payload k_fd_difference runs over the RESIDENT jobs -- those of kept trajectories
 * rewrite what their records hold; a host that uploads the listed trajectories' jobs alone touches nobody else -- and k_interpolate
 * over the list.  With KPILQR_FD_INTERP=0 the three-pass sequence runs with its record-writing passes restricted to the list (the
 * column scatter once per run of adjacent trajectories: a diagnostic path).  kpilqr_fd_interpolate_partial is KPILQR_ERR_STATE
 * before any key-points exist and while ranges are pending after kpilqr_update_keypoints; kpilqr_cost_derivs_partial makes the
 * broadcast copy of constant Jacobians as kpilqr_cost_derivs does.  On a KPILQR_FLAG_FUSED context both return KPILQR_ERR_STATE: it
 * holds no persistent records and its sweeps read the column store.  kpilqr_last_launch(ctx, 2) reports the form with ":subset"
 * appended ("fd_kp_interpolate:subset", "kp_columns_interpolate:subset", "fd_difference+interpolate:subset").
 *
 * Out of scope: the sweeps still run over the whole batch; kpilqr_generate_keypoints and kpilqr_upload_states for a subset; keeping
 * the column store, slope store and union store of kept trajectories on a KPILQR_FLAG_FUSED context; kpilqr_iterate and
 * kpilqr_iterate_streamed (whole batch); job-list payloads carried across kpilqr_update_keypoints.
 * (since: kpilqr_backward_partial, kpilqr_forward_linear_partial and kpilqr_iterate_partial sweep a listed subset -- "Sweeps of a subset".)
 * (since: kpilqr_upload_states_partial and kpilqr_generate_keypoints_partial -- "Key-point placement for a subset".) */
int  kpilqr_upload_residuals_partial(kpilqr_ctx *ctx, int count, const int *traj,
                                     const double *r, const double *r_x, const double *r_u);
int  kpilqr_upload_nominal_partial(kpilqr_ctx *ctx, int count, const int *traj, const double *u_nom);
int  kpilqr_fd_interpolate_partial(kpilqr_ctx *ctx, int count, const int *traj);
int  kpilqr_cost_derivs_partial(kpilqr_ctx *ctx, int count, const int *traj);

/* Key-point placement on the device for the whole batch (optional).
 * X [batch][T][n]: the nominal trajectory states (positions then velocities), as Optimiser::X_old. */
int  kpilqr_upload_states(kpilqr_ctx *ctx, const double *X);
/* KeypointGenerator::GenerateKeyPoints (src/KeyPointGenerator/KeyPointGenerator.cpp:76-135) for method
 * "set_interval" (:319-339), "adaptive_jerk" (:730-770 + :341-382), "adaptive_accel" (:772-795 + :341-382, dispatch
 * :98-101; thresholds = jerk_thresholds, which the placement reads for either profile) or "velocity_change" (:797-808 + :642-728)
 * on every trajectory; the lists become the context's key-points exactly as if given to
 * kpilqr_set_keypoints.  thresholds [dof] (jerk or velocity-change thresholds; NULL for set_interval), dt =
 * model time-step.  "iterative_error" interleaves host finite differences: its placement loop stays on the host and calls
 * kpilqr_keypoint_error_test per bisection level. */
int  kpilqr_generate_keypoints(kpilqr_ctx *ctx, const char *method, int min_N, int max_N,
                               const double *thresholds, double dt);
/* The error test of "iterative_error" for one bisection level of the whole batch (KeypointGenerator::CheckDOFColumnError,
 * src/KeyPointGenerator/KeyPointGenerator.cpp:550-640): intervals [n][4] = trajectory, DoF, start, end.  The host
 * differences the DoF's columns at start, (start+end)/2 and end of every pending interval (kpilqr_upload_fd +
 * kpilqr_fd_difference put them into the step records), this call says which intervals are good (1: keep, 0: split at the
 * midpoint), the host bisects the others -- placement stays a host loop because it interleaves the simulator
 * (GenerateKeyPointsIteratively :449-548), the arithmetic of a level runs here.  Synchronous. */
int  kpilqr_keypoint_error_test(kpilqr_ctx *ctx, int n, const int *intervals, int min_N, double threshold, unsigned char *good);
/* Reads the current per-DoF lists back (the host FD loop needs them): kp_offsets [batch*dof+1]; kp_times may be
 * NULL to query the size.  Returns the total number of entries (>= 0) or an error (< 0).  Synchronous. */
int  kpilqr_get_keypoints(kpilqr_ctx *ctx, int *kp_offsets, int *kp_times, int times_capacity);

/* ---- Key-point placement for a subset: states, placement and the new lists of a LIST of trajectories --------------------------
 * Device placement and partial re-linearisation together: the trajectories whose step was accepted get new states and new lists
 * placed on the device, and the by-entry payload of everybody else stays resident.  (count, traj) has the contract of the _partial
 * family in all three calls: `traj` [count] strictly increasing and within [0, batch), else KPILQR_ERR_ARG and nothing is enqueued
 * or changed; count = 0 is a no-op returning KPILQR_OK; a NULL context is KPILQR_ERR_ARG; not through a view of
 * kpilqr_iterate_streamed's chunks (KPILQR_ERR_STATE, never allocates); each call orders itself behind a streamed iteration in
 * flight.  KPILQR_VERSION is unchanged: detect the calls by their symbols.
 *
 * kpilqr_upload_states_partial: X [count][T][n], the listed trajectories' states COMPACT in `traj` order.  The rows go straight to
 * their place in the states buffer (allocated on first use, as kpilqr_upload_states allocates it), one hipMemcpyAsync per run of
 * adjacent trajectories: no staging buffer, no kernel.  The context keeps one host byte per trajectory that says whether its states
 * were ever given: a whole kpilqr_upload_states sets all of them, kpilqr_resize clears them.
 *
 * kpilqr_generate_keypoints_partial takes the methods, argument checks and dof <= 64 bound of kpilqr_generate_keypoints
 * ("iterative_error" is refused with the same message) and leaves the context exactly as kpilqr_update_keypoints(count, traj, lists)
 * would, where `lists` are bit for bit what kpilqr_generate_keypoints with the same arguments and states places for the listed
 * trajectories: the CSR merged, kept trajectories' times and by-entry payload moved to their new offsets in the second buffers, the
 * listed ranges PENDING until kpilqr_upload_fd_kp_partial / kpilqr_upload_kp_columns[_f32]_partial fills them, the union lists
 * invalid, the host mirror of the offsets valid.  The listed trajectories' flags are what the whole-batch placement sets: canonical,
 * and uniform only for set_interval.  KPILQR_ERR_STATE: before any key-points exist; while ranges are pending after an earlier
 * update; for a method other than set_interval when a listed trajectory never had states uploaded (the message names the first
 * such trajectory).  A rejected call leaves the context as it was.
 * How, and what it costs.  The placement kernel runs with `count` workgroups: workgroup i reads the states of trajectory traj[i]
 * off the device copy of the list (the one kpilqr_fd_interpolate_partial uses), a scalar load, and writes bitmask and count rows i,
 * compact.  The call then WAITS for ONE read-back of the count*dof counts -- the whole-batch call waits for its total -- so every
 * size is known exactly and no worst-case count*dof*T reservation of list times is made; the compact offsets go back up, the
 * bitmasks are expanded into the buffer kpilqr_update_keypoints uploads its caller's times to, and from there the two calls are one
 * function: costs, second buffers and the final wait of kpilqr_update_keypoints apply as written there.  With a job-list payload,
 * or with none, there is nothing to carry.
 *
 * kpilqr_get_keypoints_partial reads the listed trajectories' lists back COMPACT (the host FD loop needs them before it can fill the
 * listed trajectories' records): kp_offsets [count*dof + 1] re-based to 0, kp_times with one copy per run of adjacent trajectories.
 * Returns the number of entries of the listed trajectories (>= 0) or an error (< 0).  Synchronous, like kpilqr_get_keypoints.
 * kp_times = NULL queries the size and does not touch the device when the offsets mirror is valid (always after
 * kpilqr_set_keypoints, kpilqr_update_keypoints and kpilqr_generate_keypoints_partial; behind kpilqr_generate_keypoints the first
 * call reads the offsets back, once).  A times_capacity that is too small is KPILQR_ERR_ARG.  It works on any lists, not only
 * device-placed ones, and it is allowed while ranges are pending: it reads lists, not payload.
 *
 * Out of scope: the host shims (they place key-points on the host); the chunks of kpilqr_iterate_streamed;
 * kpilqr_keypoint_error_test for a subset; job-list payloads carried across the update; an environment switch. */
int  kpilqr_upload_states_partial(kpilqr_ctx *ctx, int count, const int *traj,
                                  const double *X /* [count][T][n], compact, traj order */);
int  kpilqr_generate_keypoints_partial(kpilqr_ctx *ctx, int count, const int *traj, const char *method,
                                       int min_N, int max_N, const double *thresholds, double dt);
int  kpilqr_get_keypoints_partial(kpilqr_ctx *ctx, int count, const int *traj,
                                  int *kp_offsets /* [count*dof + 1], starts at 0 */,
                                  int *kp_times /* or NULL */, int times_capacity);

/* Host FD results, one job per perturbed column (Differentiator::DynamicsDerivatives,
 * src/Differentiator/Differentiator.cpp:81-428 stays on the host and fills these):
 *   job_b[j], job_t[j]   trajectory and time index of the key-point
 *   job_col[j]           0..n-1 -> column of A (i: d/dqpos_i, i+dof: d/dqvel_i); n..n+m-1 -> column of B
 *   job_mode[j]          0 central (x+ - x-)/(2 eps), 1 forward (x+ - xnom)/eps, 2 backward (xnom - x-)/eps
 *   job_nom[j]           row of xnom holding the unperturbed next state (modes 1,2)
 *   xplus, xminus        [njobs][n] tangent-space next states; xnom [nnom][n]
 * One hipMemcpyAsync per array; with pinned host arrays (kpilqr_host_alloc) the call returns without waiting for them
 * (pageable arrays are waited for).  Jobs may come in any order; indices are checked on the device (see
 * kpilqr_upload_fd_slab): no host-side pass over the jobs. */
int  kpilqr_upload_fd(kpilqr_ctx *ctx, int njobs, const int *job_b, const int *job_t,
                      const int *job_col, const unsigned char *job_mode, const int *job_nom,
                      const double *xplus, const double *xminus,
                      int nnom, const double *xnom, double eps);
/* ---- asynchronous boundary: one pinned slab, no host-side loops, no stream synchronisation ---------------------------
 * The FD workers (Optimiser::WorkerComputeDerivatives, src/Optimiser/Optimiser.cpp:262-323, here
 * Differentiator::DynamicsDerivativesPlanned) write their jobs straight into ONE pinned allocation laid out as below; the
 * upload is then a single hipMemcpyAsync into an identically laid-out device slab.  Jobs may come in any order.  Indices
 * are range-checked ON THE DEVICE (a bad job is skipped); a violation is reported by the next kpilqr_sync as
 * KPILQR_ERR_ARG. */
typedef struct {
    size_t xplus, xminus, xnom;                 /* byte offsets of the double arrays [njobs][n], [njobs][n], [nnom][n] */
    size_t job_b, job_t, job_col, job_nom;      /* int arrays [njobs]                                                   */
    size_t job_mode;                            /* unsigned char array [njobs]                                          */
    size_t bytes;                               /* size of the slab                                                     */
} kpilqr_fd_layout;
int  kpilqr_fd_slab_layout(kpilqr_ctx *ctx, int njobs, int nnom, kpilqr_fd_layout *out);
int  kpilqr_upload_fd_slab(kpilqr_ctx *ctx, const void *slab, int njobs, int nnom, double eps);

/* ---- key-point ordered FD payload: no job lists at all -------------------------------------------------------------------
 * The same FD results laid out BY the key-point lists the context holds (kpilqr_set_keypoints / kpilqr_generate_keypoints +
 * kpilqr_get_keypoints): CSR entry e = position in kp_times, i.e. (trajectory b, DoF d, key-point time t = kp_times[e]),
 * and three slots per entry,
 *     kind 0: qpos_d perturbed  -> column d       of A      (Differentiator.cpp:328-428)
 *     kind 1: qvel_d perturbed  -> column d + dof of A      (:226-325)
 *     kind 2: ctrl_d perturbed  -> column d       of B      (:81-223; only d < num_ctrl, other kind-2 slots are ignored)
 * One RECORD per entry, `entry_stride` = (6n + 2) * 8 bytes, records back to back in CSR order:
 *   struct { double xplus, xminus; } x[3][n]
 *            xplus   next state after the + perturbation  (a backward-only difference: the unperturbed next state)
 *            xminus  next state after the - perturbation  (a forward-only difference:  the unperturbed next state)
 *            -- the two sides of an element side by side (`elem_stride` = 16 bytes from one element of a side to the next, xminus
 *            8 bytes behind xplus; version >= 400; versions < 400 stored the sides as two blocks of 3n doubles): the sweep that
 *            differences the payload itself fetches both with ONE 16-byte load per element
 *   int32  mode              bit k set: kind k is one-sided -> (xplus - xminus) / eps, else (xplus - xminus) / (2 eps)
 *   int32  pad[3]
 * so the host FD loop writes every perturbed next state straight to its slot, nothing carries indices, the library never
 * walks or sorts anything, and a trajectory's (or a chunk of trajectories') payload is one contiguous range.  On a KPILQR_FLAG_FUSED context (one wavefront per trajectory, or the consumer / helper wave pair up to #SIMDs / 2 trajectories) there
 * is then NO differencing kernel either: the backward sweep reads the slots of a key-point when it reaches it, forms the
 * column (the arithmetic of Differentiator.cpp:166-222,441-457, bit for bit what kpilqr_fd_difference gives) and keeps it
 * for the forward sweep.  Every other context accepts the payload too (it is differenced by a streaming kernel first).
 * The payload refers to the CURRENT key-points: upload it after them; new key-points invalidate it.  `entries` must be
 * kp_offsets[batch*dof].  One hipMemcpyAsync; with a pinned slab the call does not wait. */
typedef struct {
    size_t entry_stride;                        /* bytes of one entry record: (6n + 2) * 8                       */
    size_t xplus, xminus, mode;                 /* byte offsets inside a record: 0, 8, 6n * 8 (an int32)         */
    size_t bytes;                               /* entries * entry_stride                                        */
    size_t elem_stride;                         /* bytes between consecutive elements of xplus (and of xminus): 16; element
                                                   (kind k, row r) of xplus sits at xplus + (k * n + r) * elem_stride    */
} kpilqr_fdkp_layout;
int  kpilqr_fd_kp_layout(kpilqr_ctx *ctx, int entries, kpilqr_fdkp_layout *out);
int  kpilqr_upload_fd_kp(kpilqr_ctx *ctx, const void *slab, int entries, double eps);

/* The key-point columns themselves, for a host that has already differenced (the reference's own place for a2,
 * Differentiator.cpp:166-222,441-457, or analytic derivatives): columns [entries][3][n] in CSR entry order, kinds as above
 * (column d of A, column d + dof of A, column d of B; kind-2 slots of DoFs >= num_ctrl are ignored) -- the layout of the
 * library's key-point column store, uploaded straight into it: 3n doubles per entry instead of the 6n + 2 of the FD payload,
 * and no differencing on the device.  With the IEEE quotients (x+ - x-) / (2 eps) the gains are bit for bit those of
 * kpilqr_upload_fd_kp.  Refers to the CURRENT key-points like the FD payloads; replaces them. */
int  kpilqr_upload_kp_columns(kpilqr_ctx *ctx, const double *columns, int entries);

/* The key-point columns as FP32: half the bytes of the largest upload a host that differences itself makes every iteration (3n
 * doubles per entry; Panda reaching at T = 3000, key-points every 5 steps, 4 200 entries: 1.41 MB per trajectory, 0.71 MB as FP32;
 * the x+ / x- payload is 2.89 MB).  Opt-in: kpilqr_upload_kp_columns / _partial are unchanged.
 * Contract.  Layout, entry order, kinds, the `entries` rule, the `traj` rules and the "refers to the CURRENT key-points, replaces the
 * payload" semantics are exactly those of kpilqr_upload_kp_columns / kpilqr_upload_kp_columns_partial: columns32 [entries][3][n] in
 * CSR entry order, or the listed (= pending) trajectories' entries back to back in `traj` order; kind-2 slots of DoFs >= num_ctrl
 * are present and ignored.  Rejections are theirs too, before anything is enqueued or the context changes: a NULL context or
 * pointer, a negative count or `entries` (KPILQR_ERR_ARG), a call before key-points (KPILQR_ERR_STATE), `entries` that is not
 * kp_offsets[batch*dof] -- or not the pending trajectories' sum --, a `traj` that is not the pending set (KPILQR_ERR_ARG), a resident
 * payload of the other kind (KPILQR_ERR_STATE); not through a view of kpilqr_iterate_streamed's chunks (KPILQR_ERR_STATE: a view
 * never allocates).  Pinned / pageable behaviour as kpilqr_upload_fd_kp: the call waits for the stream only when columns32 is
 * pageable, or when the staging buffer has to grow.
 * Encoding (the CALLER's side).  A column of A is a unit vector plus O(dt): a plain (float) cast of it spends FP32's 24 bits on the
 * 1 and moves the gains by up to 2.8e-6 (profiles/columns_f32.txt), past the 1e-6 they are held to.  So the unit entry is REMOVED
 * before the cast -- the subtraction in double --; for an entry of DoF d, r = 0 .. n-1:
 *     columns32[e][0][r] = (float)(A(r, d)       - (r == d ? 1 : 0))
 *     columns32[e][1][r] = (float)(A(r, d + dof) - (r == d + dof ? 1 : 0))
 *     columns32[e][2][r] = (float) B(r, d)
 * With that the gains move by at most 2.8e-7 on the measured workloads (same profile), a small multiple of what
 * kpilqr_download_gains_f32 costs.
 * Decoding (the LIBRARY's side).  kpc[e][k][r] = (double)columns32[e][k][r], an exact widening, followed by ONE IEEE addition of
 * 1.0 at the unit row of kinds 0 and 1 (r == d, r == d + dof) and nowhere else.  FP32 subnormals widen exactly, NaN stays NaN,
 * +-inf stays +-inf, -0 stays -0 off the unit rows.  The column store then holds, bit for bit, what kpilqr_upload_kp_columns
 * would hold if it were given those decoded doubles, and the context ends in the state that call leaves (payload kind, validity
 * flags, what a later kpilqr_update_keypoints relocates, what kpilqr_fd_interpolate and the raw and non-raw sweeps read): nothing
 * downstream knows the difference.
 * How.  ONE hipMemcpyAsync of the floats into a staging buffer the context owns, then ONE launch of a streaming kernel
 * (k_kp_columns_f32, columns_f32.hip: a block row per (trajectory, DoF) list of the device CSR, 8-byte loads, 16-byte stores) on the
 * context's stream.  The partial call widens only the pending trajectories' entry ranges -- those kpilqr_upload_kp_columns_partial
 * copies into -- however scattered the list is: the kernel reads where each of them starts from the table kpilqr_update_keypoints
 * left on the device.  kpilqr_last_launch is unchanged (it describes the sweeps and the linearisation).
 * Memory cost: the staging buffer, entries*3n*4 bytes of device memory, reserved on demand and kept at the largest size asked for
 * (half the size of the column store; KPILQR_ERR_ALLOC when it cannot be had).  A context that never makes these calls allocates
 * and launches nothing for them.
 * Out of scope: the chunk pipeline (kpilqr_stream_io and kpilqr_stream_io2 are fixed structs: a streamed FP32 column route needs a
 * call of its own); FP32 for the x+ / x- payloads, residuals, residual Jacobians, nominal controls, or inside any sweep; the batch
 * shim (it uploads x+ / x-); an environment switch.  KPILQR_VERSION is unchanged: detect the calls by their symbols. */
int  kpilqr_upload_kp_columns_f32(kpilqr_ctx *ctx, const float *columns32 /* [entries][3][n] */, int entries);
int  kpilqr_upload_kp_columns_f32_partial(kpilqr_ctx *ctx, int count, const int *traj,
                                          const float *columns32 /* the listed trajectories' entries, back to back */, int entries);

/* The per-step residual Jacobians as FP32: half the bytes of the largest upload of a task whose residuals are not affine in the
 * state (such a task cannot use kpilqr_upload_residual_jacobians_const and sends r_x and r_u every time it linearises; Panda at
 * T = 3000, nr = 14: 4.71 + 2.35 = 7.06 MB per trajectory, 3.53 MB as FP32, against 1.9 MB for everything else that crosses the
 * link once the FP32 columns and the FP32 gains are on).  Opt-in: kpilqr_upload_residuals / _partial are unchanged, and a context
 * that never makes these calls allocates, copies and launches nothing for them.  (This is the transport the column paragraph
 * above lists as out of scope; it has since arrived here.)
 * Contract.  r_x32 [batch][T+1][nr][n] and r_u32 [batch][T+1][nr][m] -- for the partial call the listed trajectories' rows, compact
 * in `traj` order: [count][T+1][nr][n], [count][T+1][nr][m] -- in the layout of kpilqr_upload_residuals; NULL = not sent.  After
 * either call the context is, bit for bit and flag for flag, what kpilqr_upload_residuals(ctx, NULL, rx, ru, NULL, NULL) -- or
 * kpilqr_upload_residuals_partial(ctx, count, traj, NULL, rx, ru) -- leaves when rx[i] = (double)r_x32[i] and ru[i] =
 * (double)r_u32[i]: the r_x / r_u buffers, the end of constant-Jacobian mode behind a whole r_x32, which rows of r_x have been
 * given, r_u counted as non-zero once r_u32 is given, and with them what the fused sweeps, kpilqr_cost_derivs[_partial] and
 * kpilqr_last_launch (:ru0, :rxc) then do: nothing downstream knows the difference.  r, w_run and w_term stay with
 * kpilqr_upload_residuals: r is small and stays FP64.  Both pointers NULL is KPILQR_OK with nothing enqueued.
 * Encoding (the CALLER's side).  A plain (float) cast, round to nearest even: r_x has no unit entry that would eat the mantissa, so
 * nothing is removed or added (unlike the key-point columns above).  The library widens: dst = (double)src, an exact widening and
 * nothing else.  FP32 subnormals widen to their value, +-inf stays +-inf, -0 stays -0, NaN stays NaN.
 * What it costs in accuracy.  2^-24 (6e-8) relative per element of r_x and r_u.  On the numpy restatement of the pipeline
 * (oracle/crosscheck.py; panda T = 37 .. 3000, acrobot, pushing; dense and smooth residuals, lambda 1e-4 .. 10) K and k move by at
 * most 1.1e-7 and 8.0e-8: the 1e-6 bar the gains are held to is held for K and k, about ten times inside it.  It is NOT promised
 * for the clamped controls of a problem whose l_xx is rank-deficient (hopper, nr = 4 < n = 12, random Jacobians: U moved by 4.3e-6).
 * Refusals, each before anything is enqueued or changed: a NULL context (KPILQR_ERR_ARG); for the partial call the `traj` rules of
 * the _partial family (count < 0, a NULL list with count > 0, a list that is not strictly increasing or not within [0, batch):
 * KPILQR_ERR_ARG; count = 0: KPILQR_OK, nothing to do) and the three refusals of kpilqr_upload_residuals_partial, with its code
 * (KPILQR_ERR_STATE) and in its words: r_x32 while the context holds constant residual Jacobians; r_x32 of a subset before a whole
 * r_x; r_u32 of a subset on a context that runs without control residuals (:ru0).  Not through a view of
 * kpilqr_iterate_streamed's chunks (KPILQR_ERR_STATE: a view never allocates); not on an embedded context
 * (KPILQR_FLAG_EMBED_SHAPE: KPILQR_ERR_STATE, as listed there).
 * How.  ONE hipMemcpyAsync per array into a staging buffer the context owns, then ONE launch per array of a streaming kernel
 * (k_widen_rows, residuals_f32.hip: a block row per trajectory; 8-byte loads and 16-byte stores where a trajectory's element count
 * is even -- r_x always --, single elements where it is odd) on the context's stream.  The partial call makes no copy per run of a
 * scattered list: the kernel reads the list from its device copy and places the rows.  Pinned / pageable behaviour as
 * kpilqr_upload_kp_columns_f32: the call waits for the stream only when an array is pageable, or when the staging buffer has to
 * grow.  The calls order themselves behind a kpilqr_iterate_streamed still in flight.
 * Memory cost: the staging buffer, 4 bytes x (elements of r_x32 + r_u32) of the call -- 3.5 MB per trajectory at the headline shape
 * with both arrays --, reserved before anything is enqueued, grown on demand, kept at the largest size asked for and freed by
 * kpilqr_destroy (KPILQR_ERR_ALLOC when it cannot be had: the context is unchanged).
 * Out of scope: FP32 residual Jacobians inside the chunks of kpilqr_iterate_streamed* (a change of its own, as it was for the
 * columns); embedded contexts; r itself; a bounded staging arena; an environment switch.  KPILQR_VERSION is unchanged: detect the
 * calls by their symbols.
 * (since: kpilqr_iterate_streamed6, below, takes the per-step residual Jacobians as FP32 inside the chunks.) */
int  kpilqr_upload_residual_jacobians_f32(kpilqr_ctx *ctx, const float *r_x32 /* [batch][T+1][nr][n] or NULL */,
                                          const float *r_u32 /* [batch][T+1][nr][m] or NULL */);
int  kpilqr_upload_residual_jacobians_f32_partial(kpilqr_ctx *ctx, int count, const int *traj,
                                                  const float *r_x32 /* [count][T+1][nr][n] or NULL */,
                                                  const float *r_u32 /* [count][T+1][nr][m] or NULL */);

/* One whole iteration for the batch, PIPELINED over chunks of trajectories: chunk c's uploads, its kernels and its
 * downloads run on their own stream, so H2D(c+1), kernels(c) and D2H(c-1) overlap (and so do consecutive calls: nothing
 * here waits for the previous iteration).  Every host pointer must be pinned (kpilqr_host_alloc); NULL inputs keep what
 * is resident, NULL outputs are not downloaded.  Jobs are sorted by trajectory; traj_job_first / traj_nom_first
 * [batch+1] give the first job / nominal row of every trajectory (jobs of trajectory b reference nominal rows in
 * [traj_nom_first[b], traj_nom_first[b+1]) only).  Key-points, weights, control limits and alphas are set with the
 * ordinary calls beforehand.  Results are valid after kpilqr_sync.  nchunks = 0 lets the library choose (3: one chunk
 * per pipeline stream; the sweeps are latency-bound, so more chunks than streams only add their latency).  Uploads go
 * through the DMA engine, K and k come back through a copy kernel writing the pinned buffers: on this platform two DMA
 * directions do not overlap, a DMA upload and a kernel download do.
 * Consecutive calls overlap without a wait as long as (njobs, nnom, traj_job_first, traj_nom_first) stay the same -- the
 * usual case: same key-points, new payload.  When they differ from the iteration still in flight the call first orders
 * itself behind that whole iteration (the device slab is re-laid-out, so chunks could otherwise overwrite ranges another
 * chunk stream is still reading).  All offsets are validated before anything is enqueued. */
typedef struct {
    const void *fd_slab;                        /* kpilqr_fd_slab_layout(njobs, nnom); NULL: no new FD payload, the
                                                   resident one is swept again (its key-point columns are reused where
                                                   they exist; a payload that an ordinary upload call brought since the
                                                   last sweep is differenced first, on every kind of context)            */
    int njobs, nnom;
    const int *traj_job_first, *traj_nom_first; /* [batch+1]                                                             */
    double eps;
    const double *r, *r_x, *r_u;                /* [batch][T+1][nr], [..][nr][n], [..][nr][m]                            */
    const double *u_nom;                        /* [batch][T][m]                                                         */
    const double *lambda;                       /* [batch]                                                               */
    double *K, *k;                              /* out: [batch][T][n][m], [batch][T][m]                                  */
    double *cost_pred, *delta_J;                /* out: [batch][n_alpha], [batch]                                        */
    int *status;                                /* out: [batch]                                                          */
    const void *fd_kp_slab;                     /* key-point ordered payload (kpilqr_fd_kp_layout) instead of fd_slab; the
                                                   chunks' ranges follow from the key-points, no offset arrays needed     */
    int entries;                                /* kp_offsets[batch*dof]                                                 */
    const double *kp_columns;                   /* the key-point columns (kpilqr_upload_kp_columns) instead of an FD payload:
                                                   [entries][3][n]; version >= 301                                        */
} kpilqr_stream_io;
int  kpilqr_iterate_streamed(kpilqr_ctx *ctx, const kpilqr_stream_io *io, int pd_check_stride, int nchunks);

/* kpilqr_iterate_streamed with two options for the gains it brings down: K as FP32, and the gains of a list of trajectories alone --
 * what kpilqr_download_gains_f32 and kpilqr_download_gains_partial do for the explicit calls, inside the chunk pipeline.  The struct
 * carries its own size, so later fields can be appended: struct_size must be sizeof(kpilqr_stream_io2) as the caller compiled it,
 * else KPILQR_ERR_ARG.  `io` is the struct of kpilqr_iterate_streamed, every field with the meaning it has there; with K32 = NULL and
 * gain_traj = NULL the call IS kpilqr_iterate_streamed (one implementation, the same copies and launches in the same order).
 * The list.  gain_traj = NULL: K / K32 / k of the whole batch, as before.  Else gain_traj [gain_count], strictly increasing and within
 * [0, batch) -- the contract of kpilqr_download_gains_partial -- and the outputs are COMPACT: K (or K32) [gain_count][T][n][m] and
 * k [gain_count][T][m], the listed trajectories back to back in list order, and nothing beyond gain_count rows is written;
 * gain_count = 0 with a list: no gains come down.  gain_traj is read during the call only and may be pageable (the library keeps a
 * copy of its own).  The sweeps run over the whole batch regardless of the list, and cost_pred, delta_J and status stay whole-batch
 * outputs.  K of a trajectory whose status is non-zero is copied as it is (undefined, see kpilqr_backward).
 * K32.  out: K as FP32 in the layout of io.K; io.K and K32 are exclusive (io.K must then be NULL).  K32 must be pinned
 * (kpilqr_host_alloc) and 8-byte aligned.  The values are those of kpilqr_download_gains_f32: the IEEE round-to-nearest-even cast of
 * the resident FP64 K, bit for bit; FP32 subnormals are produced, not flushed; magnitudes above FLT_MAX become +-inf; NaN stays NaN.
 * k stays FP64.  The resident FP64 K is only read.
 * Rejections, all KPILQR_ERR_ARG, all before anything is enqueued or the context is changed (a context in the constant-Jacobian mode
 * stays in it): io2 = NULL; a wrong struct_size; io.K and K32 both given; K32 not pinned or not 8-byte aligned; gain_count < 0;
 * gain_count > 0 with gain_traj = NULL; a list that is not strictly increasing or leaves [0, batch).
 * How.  Chunks are contiguous trajectory ranges and the list increases, so a chunk's share is one slice of the list and one contiguous
 * range of the compact outputs.  ONE launch per chunk and array of a gather kernel (k_gains_out, gains.hip; 32 workgroups, as the copy
 * kernel of the FP64 route) reads the chunk's rows of the resident K / k, rounds K when K32 is asked for, and stores straight into the
 * caller's pinned buffer, on the chunk's own stream: no staging buffer, no second DMA, and it overlaps the uploads of the next chunks
 * as the FP64 copy kernel does.  A chunk without listed trajectories launches nothing for the gains.  K32 and the outputs of a list
 * take this route whatever KPILQR_PIPE_COPY says (bit 1 chooses between SDMA and the copy kernel for the FP64 whole-batch downloads
 * only).  The context keeps a device copy of the list (batch ints) and its mirror: consecutive calls overlap without a wait while
 * the list equals the one in flight; a different list first orders the call behind the iteration in flight, as differing job
 * offsets do.
 * Bytes: Panda reaching, T = 3000: 2.52 MB of gains per trajectory become 1.34 MB with K32, and proportionally fewer with a list;
 * uploads stay and share the link, so the rate gains less: measured once at B = 1024, three chunks, against the FP64 call in the same
 * process, 1.10x with K32, 1.22x with K32 of a scattered half of the batch, 1.17x with FP64 K of that half (profiles/streamed_gains.txt).
 * Out of scope: FP32 for k, for any upload or inside any sweep; uploads or sweeps of a subset inside the chunks
 * (kpilqr_iterate_streamed4 has since added the uploads); KPILQR_FLAG_UNION_KEYPOINTS inside the chunks.  KPILQR_VERSION is unchanged: detect the call by its symbol.
 * (since: the explicit calls sweep a listed subset -- "Sweeps of a subset"; the chunks still sweep every trajectory.)
 * (since: kpilqr_iterate_streamed5, below, linearises and sweeps a listed subset inside the chunks.) */
typedef struct {
    size_t struct_size;                         /* sizeof(kpilqr_stream_io2) as the caller compiled it                   */
    kpilqr_stream_io io;                        /* every field with the meaning it has for kpilqr_iterate_streamed       */
    float *K32;                                 /* out: K as FP32, layout of io.K; io.K must then be NULL                */
    int gain_count;                             /* with gain_traj: number of listed trajectories (0: no gains come down) */
    const int *gain_traj;                       /* NULL: K / K32 / k of the whole batch.  Else [gain_count], strictly increasing,
                                                   within [0, batch): K (or K32) [gain_count][T][n][m] and k [gain_count][T][m]
                                                   COMPACT, in list order                                                 */
} kpilqr_stream_io2;
int  kpilqr_iterate_streamed2(kpilqr_ctx *ctx, const kpilqr_stream_io2 *io2, int pd_check_stride, int nchunks);

/* kpilqr_iterate_streamed2 taking the key-point columns as FP32 inside the chunks -- what kpilqr_upload_kp_columns_f32 does for the
 * explicit call, in the chunk pipeline: a host that differences itself sends half the bytes of its largest upload and keeps the
 * overlap.  struct_size must be sizeof(kpilqr_stream_io3) as the caller compiled it, and io2.struct_size sizeof(kpilqr_stream_io2),
 * else KPILQR_ERR_ARG.  `io2` is the struct of kpilqr_iterate_streamed2, every field with the meaning it has there (K32 and gain_traj
 * combine freely with kp_columns32); with kp_columns32 = NULL the call IS kpilqr_iterate_streamed2 (one implementation, the same
 * copies and launches in the same order).
 * The payload.  kp_columns32 is a fourth payload kind beside io.fd_slab, io.fd_kp_slab and io.kp_columns: one payload per iteration,
 * at most one of the four may be given.  [io2.io.entries][3][n] floats in CSR entry order, io2.io.entries = kp_offsets[batch*dof] as
 * for io.kp_columns, the lists known to the host as for io.kp_columns (kpilqr_set_keypoints, or kpilqr_get_keypoints after generating
 * them; else KPILQR_ERR_STATE).  kp_columns32 must be pinned (kpilqr_host_alloc) and is read until the iteration has completed.
 * Encoding and decoding are, word for word, those of kpilqr_upload_kp_columns_f32: the caller removes A's unit entry before the
 * cast, the library widens exactly and adds 1.0 at the unit rows of kinds 0 and 1 and nowhere else; kind-2 slots of DoFs >= num_ctrl
 * are present and ignored.  After the call the context is in the state an iteration with io.kp_columns fed the decoded doubles
 * leaves (payload kind, validity flags, what a later kpilqr_update_keypoints relocates), and K, k, cost_pred, delta_J and status
 * are that iteration's bit for bit: nothing downstream knows the difference.
 * Rejections, all KPILQR_ERR_ARG, all before anything is enqueued or the context is changed (a context in the constant-Jacobian mode
 * stays in it): ctx = NULL or io3 = NULL; a wrong struct_size, outer or inner; kp_columns32 not pinned; kp_columns32 given together
 * with another payload; io2.io.entries that is not the number of key-point entries.  The refusals of kpilqr_iterate_streamed2 keep
 * their codes.
 * How.  Per chunk, on the chunk's own stream: ONE upload of the chunk's entries*3n floats into its range of the staging buffer of
 * kpilqr_upload_kp_columns_f32 (by SDMA or by the copy kernel, as KPILQR_PIPE_COPY bit 0 says for every other upload), then ONE
 * launch of k_kp_columns_f32 over the chunk's lists (columns_f32.hip), which decodes that range into the chunk's range of the
 * column store; a chunk without entries copies and launches nothing.  The staging buffer is the context's, entries*3n*4 bytes,
 * reserved before the chunks are cut (KPILQR_ERR_ALLOC when it cannot be had) and kept; a call that has to grow it first orders
 * itself behind the iteration in flight.  Consecutive calls with unchanged key-points overlap without a wait: a chunk's range of the
 * staging buffer follows from the key-points alone, so same-stream order protects it from the next call's upload.  The explicit
 * kpilqr_upload_kp_columns_f32 / _partial share the buffer and order themselves behind a streamed iteration in flight.
 * Bytes: Panda reaching, T = 3000, key-points every 5 steps: 1.41 MB of columns per trajectory become 0.71 MB; residuals, nominal
 * controls and the downloads stay and share the link (profiles/streamed_columns_f32.txt holds the byte model and what was measured).
 * Out of scope: uploads or sweeps of a subset inside the chunks; KPILQR_FLAG_UNION_KEYPOINTS inside the chunks; FP32 for x+ / x-,
 * residuals, residual Jacobians, u_nom or k, or inside any sweep; the host classes (they do not use the streamed route); any change
 * to kpilqr_stream_io or kpilqr_stream_io2; an environment switch.  KPILQR_VERSION is unchanged: detect the call by its symbol.
 * (Uploads of a subset inside the chunks have since arrived as kpilqr_iterate_streamed4, below; its sweeps still cover every trajectory.)
 * (since: the explicit calls sweep a listed subset -- "Sweeps of a subset"; the chunks still sweep every trajectory.)
 * (since: kpilqr_iterate_streamed5, below, linearises and sweeps a listed subset inside the chunks.)
 * (since: kpilqr_iterate_streamed6, below, takes the per-step residual Jacobians as FP32 inside the chunks.) */
typedef struct {
    size_t struct_size;                         /* sizeof(kpilqr_stream_io3) as the caller compiled it                   */
    kpilqr_stream_io2 io2;                      /* every field as for kpilqr_iterate_streamed2; io2.struct_size = sizeof(kpilqr_stream_io2) */
    const float *kp_columns32;                  /* the ENCODED key-point columns of kpilqr_upload_kp_columns_f32,
                                                   [io2.io.entries][3][n], pinned; NULL: the call is kpilqr_iterate_streamed2 */
} kpilqr_stream_io3;
int  kpilqr_iterate_streamed3(kpilqr_ctx *ctx, const kpilqr_stream_io3 *io3, int pd_check_stride, int nchunks);

/* kpilqr_iterate_streamed3 uploading the inputs of a LISTED SUBSET of the batch inside the chunks -- what kpilqr_update_keypoints,
 * kpilqr_upload_*_partial do for the explicit calls, in the chunk pipeline: a host that re-linearises only the trajectories whose
 * last step was accepted (src/Optimiser/iLQR.cpp:419) sends their inputs alone and keeps the overlap; everybody else repeats the
 * backward pass at a new lambda on the derivatives that are resident.  struct_size must be sizeof(kpilqr_stream_io4) as the caller
 * compiled it, io3.struct_size sizeof(kpilqr_stream_io3) and io3.io2.struct_size sizeof(kpilqr_stream_io2), else KPILQR_ERR_ARG.
 * `io3` is the struct of kpilqr_iterate_streamed3, every field with the meaning it has there; with upload_traj = NULL the call IS
 * kpilqr_iterate_streamed3 (one implementation, the same copies and launches in the same order; upload_count is then ignored
 * unless it is > 0, which is refused).
 * The list.  upload_traj [upload_count] is strictly increasing and within [0, batch) (the rules of kpilqr_download_gains_partial and
 * gain_traj); it is read during the call only and may be pageable; it is independent of gain_traj.
 * Compact inputs.  io.r [count][T+1][nr], io.r_x [count][T+1][nr][n], io.r_u [count][T+1][nr][m], io.u_nom [count][T][m]: the listed
 * trajectories' rows back to back in list order; a NULL pointer keeps what is resident; all pinned as before.  The payload: at most
 * one of io.fd_kp_slab, io.kp_columns, io3.kp_columns32 may be given; it holds the records / columns / encoded floats of the listed
 * trajectories' CSR entries back to back in list order, io.entries is the sum of their entry counts under the CURRENT lists, the
 * lists must be known to the host as for the by-entry payloads of the older calls, and the encoding of kp_columns32 is unchanged.
 * io.lambda stays [batch]: lambda changes for everybody.  All outputs keep their meaning, whole batch or gain_traj.
 * upload_count = 0 with a list: no input but lambda is copied; the sweeps and downloads run on what is resident.
 * Results and state afterwards are those of a kpilqr_iterate_streamed3 given whole-batch arrays that hold the resident bytes with the
 * listed rows / entries replaced: K, k, cost_pred, delta_J and status bit for bit, and the same payload kind, validity flags, what
 * a later kpilqr_update_keypoints relocates, and kpilqr_last_launch strings.  The sweeps, and on a context with records the
 * linearisation, still run over every trajectory of every chunk.
 * Changed key-points.  The caller first calls kpilqr_update_keypoints for the trajectories whose lists changed (an ordinary call: it
 * orders itself behind the pipeline), which leaves their ranges pending.  A streamed4 call whose payload list contains every
 * pending trajectory completes them -- a superset is fine -- and after it nothing is pending.  A list that misses a pending
 * trajectory is KPILQR_ERR_STATE naming it.
 * Rejections, all before anything is enqueued or the context is changed (a context in the constant-Jacobian mode stays in it).
 * KPILQR_ERR_ARG: ctx = NULL or io4 = NULL; a wrong struct_size, outer or inner; upload_count < 0; upload_count > 0 with a NULL list;
 * a list that is not strictly increasing or leaves the range; io.fd_slab together with a list (job lists carry their own
 * trajectory indices: out of scope); io.entries that is not the listed sum; io.eps that differs from the resident key-point
 * ordered payload's (a context has one eps, as for kpilqr_upload_fd_kp_partial).  KPILQR_ERR_STATE: a payload with a list while the
 * context holds no complete resident payload of the same kind for the trajectories not listed (kp_columns32 counts as the column
 * kind); r_x with a list in the constant-Jacobian mode, or before a whole r_x upload; r_u with a list before a whole r_u upload or
 * broadcast -- the refusals of kpilqr_upload_residuals_partial, in its words.  Every refusal of the older calls keeps its code.
 * How.  Per chunk and per array that is given, on the chunk's own stream: ONE upload of the chunk's compact slice -- the list
 * increases and chunks are contiguous ranges, so a chunk's share is one slice of the list and one contiguous range of each compact
 * input -- into a device staging region (by SDMA or by the copy kernel, as KPILQR_PIPE_COPY bit 0 says for every other upload), then
 * ONE launch of k_rows_in (rows_in.hip) that moves the rows device-to-device from staging to their trajectories' places; for the
 * by-entry payloads a row is the trajectory's entry range.  kp_columns32: one upload of the slice's floats, then k_kp_columns_f32
 * decoding straight into the listed trajectories' ranges of the column store, no FP64 intermediate.  A chunk without listed
 * trajectories copies and launches nothing for the inputs beyond lambda.
 * Overlap.  Two consecutive calls with DIFFERENT lists overlap like calls with equal lists: a staging region is addressed by the
 * chunk (its first trajectory), not by the list, so same-stream order protects it; the list's pinned mirror and device copy are a
 * ring of four, and a slot is written again behind the chunks that read it four calls earlier, never behind the iteration in flight.
 * Memory: staging as large as the whole-batch form of each input kind that was ever given with a list (r, r_x, r_u, u_nom, the
 * by-entry payload; kp_columns32 uses the staging buffer of kpilqr_upload_kp_columns_f32), reserved on the context before the
 * chunks are cut (KPILQR_ERR_ALLOC when it cannot be had) and kept, plus 8 ints per trajectory for the ring; a call that has to grow
 * a region first orders itself behind the iteration in flight.  A context that never passes a list allocates and launches nothing
 * new.
 * Bytes (a model): with a fraction f of the batch listed the upload of an iteration shrinks to f of itself plus lambda; the gains
 * still come down for everybody.  Panda reaching, T = 3000: 1.41 MB (columns) or 2.89 MB (x+-) of payload, 0.34 MB of r and 0.17 MB
 * of u_nom per trajectory, 4.7 MB of r_x with per-step Jacobians -- none of which crosses the link for a kept trajectory
 * (profiles/streamed_subset_uploads.txt).
 * Out of scope: sweeps or linearisation of a subset; job-list payloads (io.fd_slab) with a list; KPILQR_FLAG_UNION_KEYPOINTS inside
 * the chunks; the host classes and the batch shim (they do not use the streamed route); any change to kpilqr_stream_io, _io2 or
 * _io3; an environment switch.  KPILQR_VERSION is unchanged: detect the call by its symbol.
 * (since: the explicit calls sweep a listed subset -- "Sweeps of a subset"; the chunks still sweep every trajectory.)
 * (since: kpilqr_iterate_streamed5, below, linearises and sweeps a listed subset inside the chunks.)
 * (since: kpilqr_iterate_streamed6, below, takes the per-step residual Jacobians as FP32 inside the chunks.) */
typedef struct {
    size_t struct_size;                         /* sizeof(kpilqr_stream_io4) as the caller compiled it                   */
    kpilqr_stream_io3 io3;                      /* every field as for kpilqr_iterate_streamed3 (inner struct_sizes checked as there) */
    int upload_count;                           /* with upload_traj: number of listed trajectories                       */
    const int *upload_traj;                     /* NULL: whole-batch inputs, the call IS kpilqr_iterate_streamed3        */
} kpilqr_stream_io4;
int  kpilqr_iterate_streamed4(kpilqr_ctx *ctx, const kpilqr_stream_io4 *io4, int pd_check_stride, int nchunks);

/* kpilqr_iterate_streamed4 linearising and SWEEPING a LISTED SUBSET of the batch inside the chunks -- what kpilqr_iterate_partial does
 * for the explicit calls, in the chunk pipeline: the reference's loop does not sweep a finished trajectory again and a retry sweeps
 * only those that failed (src/Optimiser/iLQR.cpp:419, :435-442); a host with that active set keeps the overlap and pays for the
 * active trajectories alone.  struct_size must be sizeof(kpilqr_stream_io5) as the caller compiled it and the inner struct_sizes as
 * for kpilqr_iterate_streamed4, else KPILQR_ERR_ARG.  `io4` is the struct of kpilqr_iterate_streamed4, every field with the meaning it
 * has there unless said otherwise below; with sweep_traj = NULL the call IS kpilqr_iterate_streamed4 (one implementation, the same
 * copies and launches in the same order; sweep_count is then ignored unless it is > 0, which is refused).
 * The list.  sweep_traj [sweep_count] is strictly increasing and within [0, batch) (the rules of upload_traj and gain_traj); it is
 * read during the call only and may be pageable.
 * Semantics with a list.  Per chunk, the listed trajectories of that chunk are handled as kpilqr_iterate_partial handles them: on a
 * context with records the launches of kpilqr_fd_interpolate_partial and kpilqr_cost_derivs_partial (the latter not where the tiled
 * sweeps form the cost derivatives themselves), then the backward and the forward sweep, all for the listed alone.  No byte of an
 * unlisted trajectory's K, k, status, delta_J, cost_pred, lambda, attempts or step records is written.
 * Compact small arrays.  io.lambda [sweep_count] in list order, placed by one k_rows_in launch per chunk (NULL keeps the resident
 * lambdas); io.cost_pred [sweep_count][n_alpha], io.delta_J and io.status [sweep_count]: nothing beyond sweep_count rows is written.
 * K / K32 / k keep following gain_traj exactly as before -- without it the whole batch's resident gains -- and gain_traj is
 * independent of sweep_traj.
 * Uploads.  Inputs come with an upload_traj, which must be a subset of sweep_traj (a re-linearised trajectory is an active one): r,
 * r_x, r_u, u_nom or a payload without upload_traj, or an upload_traj entry missing from sweep_traj (the error names it), is
 * KPILQR_ERR_ARG, as is io.fd_slab.  The pending-range rule of kpilqr_iterate_streamed4 after kpilqr_update_keypoints is unchanged.
 * sweep_count = 0 with a list: nothing is swept and nothing is uploaded; the gains of gain_traj still come down.
 * State afterwards: that of kpilqr_update_keypoints' completion where ranges were pending, kpilqr_upload_*_partial for upload_traj,
 * then kpilqr_iterate_partial for sweep_traj with the compact lambdas -- payload kind, validity flags, what a later
 * kpilqr_update_keypoints relocates.  kpilqr_last_launch(ctx, 0|1|2) reports the forms with ":subset" last, on every kind of context.
 * Fused contexts.  As in the explicit listed sweeps, a listed sweep reads the column store and never differences inside the sweep.
 * The column and slope stores are reserved on the context before the chunks are cut.  Where a chunk's range of the column store is
 * not valid (a raw fd_kp payload, in this call or resident) the chunk runs the differencing and slope launches over its own entry
 * range on its own stream, whoever is listed in it; the store is then valid for everybody.  KPILQR_FLAG_UNION_KEYPOINTS is ignored.
 * Form.  What only arranges waves follows the length of the chunk's slice of the list on the chunk's share of the SIMDs, as it
 * follows the chunk's width without a list; what decides which stores exist stays the context's.
 * Lambda retry composes as in kpilqr_iterate_partial, per chunk: the schedule arms listed trajectories only, and the number of
 * attempts launched follows the chunk's slice of the compact lambdas (io.lambda = NULL: max_attempts).
 * Rejections, all before anything is enqueued or the context is changed (a context in the constant-Jacobian mode stays in it):
 * KPILQR_ERR_ARG for ctx = NULL or io5 = NULL, a wrong outer or inner struct_size, sweep_count < 0, sweep_count > 0 with a NULL list,
 * a list out of order or out of range, pd_check_stride < 1 and the cases above; KPILQR_ERR_STATE before any key-points exist.  Every
 * refusal of the older calls keeps its code.
 * How.  Everything on the chunk's own stream.  Chunks and list both increase, so a chunk's share is one slice of the list.  The view
 * the launchers get holds the context's unshifted per-trajectory pointers, the slice of the device copy of the list, the slice length
 * as its batch, the chunk's stream and its share of the SIMDs.  A chunk without listed trajectories launches nothing but its share of
 * the gain download.  The compact outputs leave by one gathering launch per chunk and array (k_rows_out, rows_in.hip) straight into
 * the caller's pinned buffer -- the route of k_gains_out: no staging buffer, no second DMA.  The list's pinned mirror and device copy
 * are a ring of four as for upload_traj: two consecutive calls with different sweep lists overlap without a wait.  Memory: 4 ints
 * per trajectory on the device and as many pinned for that ring, reserved by the first call with a non-empty sweep list; a context that never passes one allocates and
 * launches nothing new.
 * Out of scope: differencing inside a listed sweep, or proportional to the list; job-list payloads with any list;
 * KPILQR_FLAG_UNION_KEYPOINTS in the chunks; the host classes and the batch shim; any change to kpilqr_stream_io ... _io4; an
 * environment switch.  KPILQR_VERSION is unchanged: detect the call by its symbol.  (profiles/streamed_subset_sweeps.txt holds the
 * byte and launch model and says what was measured.)
 * (since: kpilqr_iterate_streamed6, below, takes the per-step residual Jacobians as FP32 inside the chunks.) */
typedef struct {
    size_t struct_size;                         /* sizeof(kpilqr_stream_io5) as the caller compiled it                   */
    kpilqr_stream_io4 io4;                      /* every field as for kpilqr_iterate_streamed4 (inner struct_sizes checked as there) */
    int sweep_count;                            /* with sweep_traj: number of listed trajectories                        */
    const int *sweep_traj;                      /* NULL: every trajectory is swept, the call IS kpilqr_iterate_streamed4 */
} kpilqr_stream_io5;
int  kpilqr_iterate_streamed5(kpilqr_ctx *ctx, const kpilqr_stream_io5 *io5, int pd_check_stride, int nchunks);

/* kpilqr_iterate_streamed5 taking the per-step residual Jacobians as FP32 inside the chunks -- what
 * kpilqr_upload_residual_jacobians_f32[_partial] do for the explicit calls, in the chunk pipeline: a host whose residuals are not
 * affine in the state sends half the bytes of its largest upload and keeps the overlap, the subset uploads of upload_traj and the
 * subset sweeps of sweep_traj.  struct_size must be sizeof(kpilqr_stream_io6) as the caller compiled it and the inner struct_sizes as
 * for kpilqr_iterate_streamed5, else KPILQR_ERR_ARG.  `io5` is the struct of kpilqr_iterate_streamed5, every field with the meaning it
 * has there; with r_x32 = NULL and r_u32 = NULL the call IS kpilqr_iterate_streamed5 (one implementation, the same copies and launches
 * in the same order).
 * The arrays.  r_x32 [batch][T+1][nr][n] and r_u32 [batch][T+1][nr][m] in the layout of io.r_x / io.r_u; with upload_traj the listed
 * trajectories' rows, [upload_count][T+1][nr][n] and [upload_count][T+1][nr][m], compact in list order, as io.r_x / io.r_u are there;
 * NULL = not sent.  Both must be pinned (kpilqr_host_alloc) and 8-byte aligned, and are read until the iteration has completed.
 * Per array, one transport per call: io.r_x together with r_x32, or io.r_u together with r_u32, is KPILQR_ERR_ARG; FP64 r_x beside
 * r_u32, and the reverse, is allowed.  They combine with every other option of the older structs: any payload kind including
 * kp_columns32, K32, gain_traj, upload_traj, sweep_traj, the lambda retry.
 * Encoding and decoding are, word for word, those of kpilqr_upload_residual_jacobians_f32: the caller makes a plain (float) cast,
 * the library widens exactly, dst = (double)src; FP32 subnormals widen to their value, +-inf stays +-inf, -0 stays -0, NaN stays
 * NaN.  Results and state afterwards are, bit for bit, those of a kpilqr_iterate_streamed5 given FP64 io.r_x / io.r_u that hold the
 * widened floats: the r_x / r_u buffers, K, k, cost_pred, delta_J, status and the kpilqr_last_launch strings (:ru0, :rxc); a whole
 * r_x32 ends the constant-Jacobian mode, r_u32 counts r_u as non-zero -- recorded behind every check that can still reject the call.
 * Lists.  With upload_traj the three refusals of kpilqr_upload_residuals_partial apply, with its code (KPILQR_ERR_STATE) and in its
 * words: r_x32 of a subset while the context holds constant residual Jacobians; r_x32 of a subset before a whole r_x; r_u32 of a
 * subset on a context that runs without control residuals (:ru0).  With sweep_traj the rule of kpilqr_iterate_streamed5 holds for
 * the new arrays too: inputs come with an upload_traj inside sweep_traj, r_x32 or r_u32 without one is KPILQR_ERR_ARG.
 * Rejections, all before anything is enqueued or the context is changed (a context in the constant-Jacobian mode stays in it):
 * KPILQR_ERR_ARG for ctx = NULL or io6 = NULL, a wrong outer or inner struct_size, r_x32 or r_u32 not pinned or not 8-byte aligned,
 * an array given through both transports, and the sweep_traj rule above; KPILQR_ERR_STATE for the three refusals of a subset.  Not
 * on an embedded context (KPILQR_FLAG_EMBED_SHAPE: KPILQR_ERR_STATE, as listed there).  Every refusal of the older calls keeps its
 * code.
 * How.  Per chunk, on the chunk's own stream, ONE launch serves BOTH arrays (k_widen_jacobians, residuals_f32.hip; the sweeps are
 * latency-bound, so a chunk does not pay two launches where one does): a block row is a trajectory of the chunk -- without a list
 * the chunk's own, with upload_traj the chunk's slice of the device copy of the list, so a scattered list costs no copy per run --
 * and a split of the grid's x range selects the array; an array that is not given costs no block.  r_x is widened in pairs (8-byte
 * loads, 16-byte stores; n = 2 dof), r_u in pairs where (T+1)*nr*m is even and in single elements (4-byte loads, 8-byte stores)
 * where it is odd: a chunk's slice of r_u32 can then start on an odd float, and nothing beyond 4-byte alignment is assumed of it.
 * The source follows KPILQR_PIPE_COPY bit 0, as every other upload does.  Uploads by SDMA (the default): ONE copy per array of the
 * chunk's slice into the staging buffer of kpilqr_upload_residual_jacobians_f32, laid out [r_x32 | r_u32] at whole-batch size, where
 * the chunk's first trajectory's rows would land, with or without a list; then the launch.  Uploads by kernel (bit 0 set): the
 * launch reads the caller's pinned floats itself; no staging buffer is reserved or touched and there is no second pass over device
 * memory -- which is why the arrays must be 8-byte aligned.  A chunk without rows copies and launches nothing for the Jacobians.
 * Overlap.  A region of the staging buffer is addressed by the chunk alone, so same-stream order protects it from the next call's
 * upload whatever that call lists: consecutive calls overlap without a wait.  The explicit kpilqr_upload_residual_jacobians_f32 /
 * _partial share the buffer and order themselves behind a streamed iteration in flight.
 * Memory: the staging buffer, 4 bytes x batch x (T+1) x nr x (n + m), reserved on the context before the chunks are cut
 * (KPILQR_ERR_ALLOC when it cannot be had) and kept; a call that has to grow it first orders itself behind the iteration in flight.
 * A context that never passes r_x32 / r_u32 allocates and launches nothing new.
 * Bytes: Panda reaching, T = 3000, nr = 14: 7.06 MB of residual Jacobians per trajectory become 3.53 MB; r, u_nom, the payload and
 * the downloads stay and share the link (profiles/streamed_residual_jacobians_f32.txt holds the byte model and what was measured).
 * Out of scope: FP32 for r, u_nom or k, or inside any sweep; the host classes and the batch shim (they do not use the streamed
 * route); embedded contexts; a bounded staging arena; any change to kpilqr_stream_io ... _io5; an environment switch.
 * KPILQR_VERSION is unchanged: detect the call by its symbol. */
typedef struct {
    size_t struct_size;                         /* sizeof(kpilqr_stream_io6) as the caller compiled it                   */
    kpilqr_stream_io5 io5;                      /* every field as for kpilqr_iterate_streamed5 (inner struct_sizes checked as there) */
    const float *r_x32;                         /* [batch][T+1][nr][n], or with upload_traj [upload_count][T+1][nr][n] compact in
                                                   list order; NULL: not sent                                             */
    const float *r_u32;                         /* [batch][T+1][nr][m], or compact likewise; NULL: not sent               */
} kpilqr_stream_io6;
int  kpilqr_iterate_streamed6(kpilqr_ctx *ctx, const kpilqr_stream_io6 *io6, int pd_check_stride, int nchunks);

/* Differencing tail of Differentiator::DynamicsDerivatives (:166-222,286-321,386-423,441-457):
 * writes the key-point columns of A and B. */
int  kpilqr_fd_difference(kpilqr_ctx *ctx);
/* KeypointGenerator::InterpolateDerivatives (src/KeyPointGenerator/KeyPointGenerator.cpp:840-954). */
int  kpilqr_interpolate(kpilqr_ctx *ctx);
/* kpilqr_fd_difference followed by kpilqr_interpolate: the resident FD payload -> A, B of every step, i.e. the differencing tail
 * of Differentiator::DynamicsDerivatives (src/Differentiator/Differentiator.cpp:166-222,441-457) and
 * KeypointGenerator::InterpolateDerivatives (src/KeyPointGenerator/KeyPointGenerator.cpp:840-954) in one call.  With a key-point
 * ordered payload (kpilqr_upload_fd_kp) or a column payload (kpilqr_upload_kp_columns) it is ONE pass over the step records that
 * fetches and differences a segment's endpoints from the payload (k_fd_kp_interpolate): the key-point column store is neither
 * written nor read, and every record is written once.  With job lists (kpilqr_upload_fd / _slab) it runs the two calls.  The
 * records hold bit for bit what the two calls leave there, including what they leave alone (steps outside a DoF list's first /
 * last key-point, B columns of actuators beyond the DoFs, the cost blocks).  On a KPILQR_FLAG_FUSED context the step records are
 * allocated on demand, as for kpilqr_interpolate.  KPILQR_ERR_STATE before kpilqr_set_keypoints / kpilqr_generate_keypoints.
 * Asynchronous on the context's stream.  kpilqr_iterate and kpilqr_iterate_streamed linearise the same way on a context with
 * step records; kpilqr_last_launch(ctx, 2) reports the form.  KPILQR_VERSION is unchanged: detect the entry point by its symbol. */
int  kpilqr_fd_interpolate(kpilqr_ctx *ctx);

/* Optimiser::FilterDynamicsMatrices (src/Optimiser/Optimiser.cpp:340-406, run from GenerateDerivatives :105-107 when
 * the task sets `filtering`): rows dof..2dof-1 of every A[t], filtered along time in place, after
 * kpilqr_interpolate.  method "low_pass" (coefs[0] = lowPassACoefficient, Optimiser.h:219) or "FIR"
 * (coefficients, Optimiser.h:220; at most 16).  Not available on a KPILQR_FLAG_FUSED context (the fused sweeps
 * re-interpolate from the key-point columns). */
int  kpilqr_filter_dynamics(kpilqr_ctx *ctx, const char *method, const double *coefs, int ncoef);

/* ---- STEP 1c: cost derivatives -----------------------------------------------------------
 * Residuals and their host-side FD Jacobians (Differentiator::ResidualDerivatives stays on the
 * host): r [batch][T+1][nr], r_x [batch][T+1][nr][n], r_u [batch][T+1][nr][m]; residual weights
 * w_run / w_term [nr] (struct residual, include/StdInclude.h:82-88).  Any pointer may be NULL to
 * keep what is already resident.  The buffers start zeroed: a task whose residuals do not depend on the controls
 * (r_u = 0: reaching, the pushing tasks) never passes r_u, and the fused sweeps then leave the control-residual
 * products out (l_uu = l_u = 0 exactly).
 * All T+1 rows of r must hold finite numbers, the last one (t = T) included, as the reference's do (it evaluates the residuals
 * at every t = 0..T, src/Optimiser/Optimiser.cpp:217-236): with an ODD residual count the one-tile sweeps fetch a row of r in
 * 16-byte pairs, and the last pair of row t reaches one element into row t+1 -- under a zero weight, which keeps a finite
 * number out of every result and would not keep a NaN out. */
int  kpilqr_upload_residuals(kpilqr_ctx *ctx, const double *r, const double *r_x, const double *r_u,
                             const double *w_run, const double *w_term);
/* CONSTANT residual Jacobians: one r_x [nr][n] (and one r_u [nr][m], or NULL for r_u = 0) that holds at every step of every
 * trajectory -- a task whose residuals are affine in the state and free of the controls, e.g. reaching: r = [q - q*, qdot],
 * r_x = selector rows, r_u = 0 (src/ModelTranslator/Reaching.cpp:43-54; the host then skips
 * Differentiator::ResidualDerivatives, src/Differentiator/Differentiator.cpp:464-663, altogether).  Uploaded ONCE per
 * context instead of T+1 copies per trajectory and iteration; on a KPILQR_FLAG_FUSED context with one wavefront per
 * trajectory (batch > #SIMDs / 4) and r_u = NULL the sweeps keep the matrix in registers and read no r_x from memory at all
 * (Panda reaching, T = 3000: 5.0 of the 8.1 MB a trajectory's backward sweep reads, 5.0 of 9.1 MB forward).  Every other
 * kernel family sees the same values through a broadcast copy made on demand, and then K, k, delta_J and the predicted costs
 * are bit for bit those of the same matrix given per step through kpilqr_upload_residuals (which, with r_x != NULL, also ends
 * the constant mode).  The sweeps that keep the matrix in registers (kpilqr_last_launch: "...:rxc") also keep the constant
 * block l_xx = r_x' W r_x as a resident tile and add l_x = r_x' W r to it with ONE matrix product per step instead of four
 * (version >= 410): the same numbers in another accumulation order -- gains identical, k / delta_J / costs within ~1e-15
 * relative of the per-step form (tests hold 1e-12).  The uniform one-wave backward sweep at n = 14, m = 7 forms Q_uu, Q_ux and
 * Q_xx from two matrix products on packed tiles instead of three ("...:w1:...:uni"): Q_uu and Q_ux keep their bits for a given value
 * function, V' moves at rounding level, so K, k, delta_J and the costs agree with the general form and with earlier versions to
 * ~1e-15 relative, not bit for bit; the two payload kinds still give each other's bits.  The uniform one-wave backward sweeps of
 * every shape symmetrise Q_xx in front of the gains instead of V' behind them: V' carries the rounding asymmetry of one matrix
 * product, and the same ~1e-15 statement holds against the general form, the wave pairs and earlier versions.  A call that is rejected (bad argument, unpinned buffer) leaves the mode
 * as it was.  version >= 400. */
int  kpilqr_upload_residual_jacobians_const(kpilqr_ctx *ctx, const double *r_x, const double *r_u);
/* ModelTranslator::CostDerivativesFromResiduals (src/ModelTranslator/ModelTranslator.cpp:552-583)
 * over the loop of Optimiser::ComputeCostDerivatives (src/Optimiser/Optimiser.cpp:202-211),
 * including the terminal-weight re-write of t = T-1. */
int  kpilqr_cost_derivs(kpilqr_ctx *ctx);
/* ModelTranslator::CostFunction (:314-327) summed over the horizon as RolloutTrajectory does
 * (src/Optimiser/iLQR.cpp:202-254): cost[b] = sum_{t<T-1} w_run.r_t^2 + w_term.r_{T-1}^2. */
int  kpilqr_trajectory_cost(kpilqr_ctx *ctx, double *cost /*[batch]*/);

/* ---- STEP 2: backward pass ----------------------------------------------------------------
 * iLQR::BackwardsPassQuuRegularisation + CheckMatrixPD (src/Optimiser/iLQR.cpp:535-670).
 * lambda [batch]; pd_check_stride = 100 in the reference.  status[b] = 0 ok, t+1 = first step
 * whose Q_uu + lambda I failed the Cholesky test; delta_J [batch].  status / delta_J may be NULL
 * (results stay on the device, KPILQR_BUF_STATUS / KPILQR_BUF_DELTA_J).  A trajectory with status != 0 has stopped at that
 * step (the reference returns false there and retries at a larger lambda, iLQR.cpp:435-442): its gains below that step, its
 * delta_J and the outputs of a kpilqr_forward_linear that follows are UNDEFINED for that trajectory until a backward pass
 * succeeds (on a fused context its key-point columns may be differenced only down to that step).  With a schedule set by
 * kpilqr_set_lambda_retry (below) the call retries such a trajectory itself, at a raised lambda. */
int  kpilqr_backward(kpilqr_ctx *ctx, const double *lambda, int pd_check_stride,
                     int *status, double *delta_J);
/* ---- Lambda retry: the failure side of the reference's lambda schedule behind the ABI ----------------------------------------
 * The reference retries a backward pass whose Q_uu + lambda I failed the Cholesky test at lambda * lambdaFactor and gives up above
 * maxLambda (src/Optimiser/iLQR.cpp:435-442, UpdateLambda :636-657).  Without a schedule that loop is the caller's: backward, sync,
 * look at status, backward again for the whole batch.  With one, every call that runs a backward sweep -- kpilqr_backward,
 * kpilqr_iterate, kpilqr_iterate_streamed and kpilqr_iterate_streamed2 (per chunk) -- runs it on the device, per trajectory:
 *     sweep at lambda; status == 0: settled.  Otherwise lambda' = lambda * factor (ONE IEEE multiply); lambda' > max_lambda: give
 *     up; otherwise, while fewer than max_attempts sweeps have run in this call, sweep again at lambda'.
 * Opt-in: set once on the context, like key-points, weights, limits and alphas (kpilqr_stream_io / _io2 are unchanged); NULL turns it
 * off, the default.  Without a schedule no copy, launch or result differs from a library without these calls.
 * After the call, per trajectory: the RESIDENT lambda is the lambda of its last sweep (lambda_used; a later call with lambda = NULL
 * starts from it), attempts is the number of sweeps it ran, and status, delta_J, K, k and the key-point columns a raw sweep leaves
 * behind are those of its last sweep.  A settled trajectory is never swept again within the call: its outputs are the bits of its
 * successful sweep.  One that gave up or ran out of attempts has the failing step of its last sweep in status and everything else
 * undefined, as above.  The success side of UpdateLambda (/ factor, the min_lambda clamp) stays with the caller, who derives its
 * state from (status, lambda_used, attempts):
 *     status == 0                                             valid backward pass at lambda_used; next lambda = max(lambda_used / factor, min_lambda)
 *     status != 0 and lambda_used * factor >  max_lambda      lambda exit (the reference clamps lambda to maxLambda and stops)
 *     status != 0 and lambda_used * factor <= max_lambda      out of attempts: call again -- with lambda = NULL the call starts at the resident
 *                                                             lambda_used (that sweep fails again) and carries on up the schedule; a
 *                                                             caller that passes lambda_used * factor saves the repeated sweep
 * (lambda_used * factor computed by the caller in double is the value the device compared.)
 * How.  Every backward kernel has a gated twin that takes `gate` [batch] and leaves at its first statement where gate[b] == 0;
 * between two attempts ONE small kernel (k_lambda_retry, lambda_retry.hip) reads status, advances lambda, counts the attempt and
 * writes the gate.  The first attempt launches the kernels without the gate: it is the launch of a context without a schedule
 * (behind one small kernel that sets every trajectory's count to 1).  The number of attempts launched is the
 * longest run the schedule allows from the lambdas the caller passed (for the streamed calls: a chunk's own slice of io.lambda),
 * computed on the host with the same multiply and capped by max_attempts; with lambda = NULL it is max_attempts.  What runs before
 * the sweep (column store, slopes, broadcast Jacobians) runs once; a retried raw sweep differences its payload again.
 * kpilqr_set_lambda_retry: KPILQR_ERR_ARG -- before anything changes -- for a struct_size that is not this library's, a factor that is
 * not finite and > 1, a max_lambda that is not finite and > 0, max_attempts outside 1 .. 64; enqueues nothing.  kpilqr_resize keeps
 * the schedule.  kpilqr_backward_stats ignores it (one instrumented sweep).
 * kpilqr_download_lambda_retry: lambda_used [batch], attempts [batch] of the last backward pass under the schedule; either may be
 * NULL.  Asynchronous on the context's stream, behind a streamed iteration in flight; valid after kpilqr_sync.  KPILQR_ERR_STATE
 * while no schedule is set or before any backward sweep ran under it.
 * KPILQR_VERSION is unchanged: detect the calls by their symbols. */
typedef struct {
    size_t struct_size;   /* sizeof(kpilqr_lambda_retry) as compiled, else KPILQR_ERR_ARG */
    double factor;        /* lambdaFactor (10): finite and > 1 */
    double max_lambda;    /* maxLambda (10): finite and > 0 */
    int    max_attempts;  /* sweeps per trajectory and call, the first included: 1 .. 64 */
} kpilqr_lambda_retry;
int  kpilqr_set_lambda_retry(kpilqr_ctx *ctx, const kpilqr_lambda_retry *sched /* NULL: off */);
int  kpilqr_download_lambda_retry(kpilqr_ctx *ctx, double *lambda_used /*[batch]*/, int *attempts /*[batch]*/);
/* Diagnostic: the backward pass of a KPILQR_FLAG_FUSED context with counters.  The explicit inverse the reference forms at
 * every step (iLQR.cpp:597-600) is carried along the sweep and refreshed on the matrix core; how much work a step needs is
 * data dependent (and a launch lasts as long as its slowest wavefront).  hist [batch][6] = steps whose inverse came from:
 * [0] the third-order refresh alone, [1..3] that plus 1 / 2 / 3 second-order steps, [4] the LDL' factorisation (first step,
 * every pd_check_stride-th step, re-seeds), [5] Eigen's pivoted LDLT restated (indefinite Q_uu + lambda I on an unchecked
 * step).  K, k, delta_J, status as kpilqr_backward; lambda as last given.  Synchronous.  Ignores kpilqr_set_lambda_retry: one sweep. */
int  kpilqr_backward_stats(kpilqr_ctx *ctx, int pd_check_stride, int *hist);
/* K [batch][T][n][m] (column-major m x n), k [batch][T][m]; either may be NULL. */
int  kpilqr_download_gains(kpilqr_ctx *ctx, double *K, double *k);
/* K as FP32: half the bytes of the largest download a re-linearising host makes every iteration (K is T*n*m*8 bytes per trajectory,
 * Panda reaching at T = 3000: 2.35 MB of the 2.52 MB of K and k; 1.18 MB as FP32).  Opt-in: the FP64 calls above are unchanged.
 * Contract.  Layout, compactness and the `traj` rules are exactly those of kpilqr_download_gains / kpilqr_download_gains_partial:
 * K32 [batch][T][n][m] (or [count][T][n][m], the listed trajectories back to back in `traj` order), k [batch][T][m] (or
 * [count][T][m]); `traj` [count] strictly increasing and within [0, batch), else KPILQR_ERR_ARG and nothing is enqueued; count = 0 is
 * a no-op returning KPILQR_OK; either pointer may be NULL; a NULL context is KPILQR_ERR_ARG; not through a view of
 * kpilqr_iterate_streamed's chunks (KPILQR_ERR_STATE: a view never allocates).  Asynchronous on the context's stream: outputs are
 * valid after kpilqr_sync (the call waits for the stream only when `traj` is pageable, as kpilqr_fd_interpolate_partial does, or when
 * the float buffer has to grow).
 * Precision.  K32[i] is the IEEE round-to-nearest-even conversion of the FP64 gain K[i], bit for bit what the C cast (float) gives:
 * at most 2^-24 (6e-8) relative per element, against the 1e-6 the gains are held to; results in the FP32 subnormal range are
 * produced, not flushed; magnitudes above FLT_MAX become +-inf; NaN stays NaN.  k stays FP64 and is the same copy as in the FP64
 * calls (7 % of the bytes, and it enters the control unscaled by a small state difference).  The resident FP64 K is never written:
 * kpilqr_download_gains*, kpilqr_forward_linear, kpilqr_dof_importance* and KPILQR_BUF_K see the same bits before and after.
 * How.  ONE launch of a streaming kernel (k_gains_f32, gains.hip) gathers the listed trajectories' K -- however scattered the list
 * is: it reads the trajectory of a block row from the device copy of the list kpilqr_fd_interpolate_partial uses -- and rounds it
 * into a compact float buffer; then ONE hipMemcpyAsync of that buffer, and the usual copies for k.
 * Memory cost: the float buffer, count*T*n*m*4 bytes of device memory owned by the context, reserved on demand and kept at the
 * largest size asked for (whole batch: half the size of K; KPILQR_ERR_ALLOC when it cannot be had).
 * Out of scope: kpilqr_iterate_streamed (kpilqr_stream_io is a fixed struct of this ABI version: its K stays FP64); FP32 for k, for
 * any upload, or inside any sweep; an environment switch.  KPILQR_VERSION is unchanged: detect the calls by their symbols.
 * (The chunk pipeline has a call of its own that brings K down as FP32: kpilqr_iterate_streamed2, with a struct that can grow.) */
int  kpilqr_download_gains_f32(kpilqr_ctx *ctx, float *K32 /* [batch][T][n][m] */, double *k /* [batch][T][m] */);
int  kpilqr_download_gains_f32_partial(kpilqr_ctx *ctx, int count, const int *traj,
                                       float *K32 /* [count][T][n][m] */, double *k /* [count][T][m] */);

/* iLQR_SVR::LeastImportantDofs on the gains of the last backward pass, both of the reference's measures, with no download of K.
 * Asynchronous on the context's stream (sums valid after kpilqr_sync); KPILQR_ERR_ARG for a NULL argument or
 * sampling_k_interval < 1.  Sums of a trajectory whose last backward pass has status != 0 are undefined.  The state-vector
 * resize a removal triggers is kpilqr_resize.
 * "Sampling and summing" branch (src/Optimiser/iLQR_SVR.cpp:952-968): sums [batch][dof] = (sum over t = 0, s, 2s, ... < T
 * and controls j of |K[t](j,i)| + |K[t](j,i+dof)|) / T. */
int  kpilqr_dof_importance(kpilqr_ctx *ctx, int sampling_k_interval, double *sums);
/* Singular-vector branch (:902-950): K[t] = U S V', sums [batch][dof] = (sum over t = 0, s, 2s, ... < T and the min(3, m)
 * largest singular triplets k of |V(i,k) S_k| + |V(i+dof,k) S_k|) / T, the SVD being host/SVR.cpp's one-sided Jacobi
 * (ThinSVD).  Bit-identical with host/SVR.cpp's DofImportance when n <= 16 and n * m' <= 128 (m' = m rounded up to a power
 * of two); otherwise equal to rounding.  KPILQR_ERR_ARG also when (n + 1) * m > 8192 (W of one step
 * does not fit the 64 KB of LDS of one wavefront).  Staging of up to 256 MB is held by the context.  Detect the entry point by its symbol. */
int  kpilqr_dof_importance_svd(kpilqr_ctx *ctx, int sampling_k_interval, double *sums);

/* ---- STEP 3: forward pass over the line-search alphas ----------------------------------------
 * Nominal controls U_old [batch][T][m] and ModelTranslator::ReturnControlLimits [2*m] = lo,hi pairs. */
int  kpilqr_upload_nominal(kpilqr_ctx *ctx, const double *u_nom, const double *ctrl_lim);
/* Control law + clamp of iLQR::ForwardsPassParallel (src/Optimiser/iLQR.cpp:876-890) on the
 * linearised model, scored with the quadratic cost model (declared semantic change, DESIGN.md
 * section 2).  alphas [n_alpha]; cost_pred [batch][n_alpha] = predicted cost CHANGE;
 * U_alpha [batch][n_alpha][T][m] or NULL. */
int  kpilqr_forward_linear(kpilqr_ctx *ctx, const double *alphas, double *cost_pred, double *U_alpha);

/* ---- one whole iteration (STEP 1b + 1c + 2 + 3) enqueued back to back ------------------------ */
int  kpilqr_iterate(kpilqr_ctx *ctx, const double *lambda, int pd_check_stride, const double *alphas);

/* ---- Sweeps of a subset: STEP 2, STEP 3 and the whole iteration over a LIST of trajectories ------------------------------------
 * kpilqr_backward / kpilqr_forward_linear / kpilqr_iterate for the listed trajectories alone: finished trajectories are not swept
 * again, a retry sweeps the trajectories that failed.  (count, traj) has the contract of the _partial family: `traj` [count] strictly
 * increasing and within [0, batch), else KPILQR_ERR_ARG and nothing is enqueued or changed; count = 0 is a no-op returning KPILQR_OK;
 * count < 0, count > 0 with a NULL list and a NULL context are KPILQR_ERR_ARG; not through a view of kpilqr_iterate_streamed's chunks
 * (KPILQR_ERR_STATE); each call orders itself behind a streamed iteration in flight and waits for the stream only when `traj` is
 * pageable.  pd_check_stride < 1 is KPILQR_ERR_ARG.
 * Compact layouts.  Host arrays are COMPACT: the listed trajectories' rows back to back in `traj` order -- lambda [count] (NULL: the
 * resident lambdas), status [count], delta_J [count], cost_pred [count][n_alpha], U_alpha [count][n_alpha][T][m]; each may be NULL.
 * Per listed trajectory K, k, status, delta_J, cost_pred, the resident lambda and U_alpha are bit for bit what a context holding
 * exactly the listed trajectories (batch = count, the same inputs, flags and environment) produces.  (A sweep that fails its PD
 * check stops at the failing step, as in kpilqr_backward: status says so, and the gains of the steps it did not reach keep what they held.)
 * No byte of an unlisted trajectory is written: its K, k, status, delta_J, cost_pred, lambda, attempts and step records keep what
 * they hold.
 * Form.  What only arranges waves follows `count`, as it follows the batch in the whole-batch calls: the wave pairs / triple / one
 * wave per trajectory of the fused sweeps, their exclusive-SIMD twins, the default of KPILQR_TILED_FSC.  What decides which stores
 * exist or are valid stays the context's: the a6 form of the tiled sweeps, ru0, rxc, the device flag for uniform lists.  The diagnostic
 * environment switches force forms as they do for the whole batch.  kpilqr_last_launch(ctx, 0 | 1) reports the form that ran with
 * ":subset" appended last.
 * Fused contexts: a subset sweep reads the column store and never differences inside the sweep.  A column store that is not valid
 * is differenced for the WHOLE batch first (the launch of kpilqr_fd_difference, with the slopes per-DoF lists need) and is then valid
 * for everybody.  KPILQR_FLAG_UNION_KEYPOINTS is ignored, as kpilqr_backward_stats ignores it.  Before any key-points exist, and while
 * ranges are pending after kpilqr_update_keypoints, the calls return KPILQR_ERR_STATE.
 * Contexts with records: the caller's contract is that of kpilqr_fd_interpolate_partial -- the listed trajectories' records hold a
 * complete linearisation.  kpilqr_iterate_partial runs kpilqr_fd_interpolate_partial, kpilqr_cost_derivs_partial (not where the tiled
 * sweeps form the cost derivatives themselves), the backward and the forward sweep; on a fused context the two sweeps only.  It sets
 * kpilqr_last_launch(ctx, 2) as kpilqr_iterate does, with ":subset" appended.
 * Lambda retry.  kpilqr_set_lambda_retry composes: the schedule runs per LISTED trajectory; an unlisted trajectory is never armed,
 * whatever status an earlier sweep left it; the attempts launched follow the compact lambdas (lambda = NULL: max_attempts).
 * kpilqr_download_lambda_retry stays a whole-batch read of what is resident.
 * How, and what it costs.  ONE launch per sweep kernel with `count` workgroups: workgroup i reads its trajectory from the device copy
 * of the list (the one kpilqr_fd_interpolate_partial uses), a scalar load.  The backward sweeps run through the lambda retry twins of
 * their kernels, which take the list beside the gate; the forward sweeps through listed twins of theirs; the kernels of the
 * whole-batch calls are unchanged.  lambda, status, delta_J and cost_pred cross with ONE copy each and one small placing or gathering
 * launch (rows_in.hip), however scattered the list is, through a staging buffer of count * (20 + 8 n_alpha) bytes reserved by the first
 * such call; U_alpha, a debug output, goes as one copy per run of adjacent trajectories out of a whole-batch staging area.  A context
 * that never makes these calls allocates and launches nothing for them.
 * Out of scope: the chunk pipeline (a streamed iteration sweeps the whole batch); differencing inside a listed sweep; keeping the
 * column store, slope store or union store of kept trajectories across kpilqr_update_keypoints; kpilqr_backward_stats,
 * kpilqr_generate_keypoints and kpilqr_upload_states for a subset; an environment switch.  kpilqr_allreduce_linesearch sums whatever
 * cost_pred and status are resident, the rows an earlier sweep left for unlisted trajectories included.
 * (since: kpilqr_upload_states_partial and kpilqr_generate_keypoints_partial -- "Key-point placement for a subset".)
 * KPILQR_VERSION is unchanged: detect the calls by their symbols. */
int  kpilqr_backward_partial(kpilqr_ctx *ctx, int count, const int *traj, const double *lambda /* [count] or NULL */,
                             int pd_check_stride, int *status /* [count] */, double *delta_J /* [count] */);
int  kpilqr_forward_linear_partial(kpilqr_ctx *ctx, int count, const int *traj, const double *alphas,
                                   double *cost_pred /* [count][n_alpha] */, double *U_alpha /* [count][n_alpha][T][m] or NULL */);
int  kpilqr_iterate_partial(kpilqr_ctx *ctx, int count, const int *traj, const double *lambda /* [count] or NULL */,
                            int pd_check_stride, const double *alphas);

/* ---- several GPUs: trajectories are sharded, one context (and one process or thread) per GPU; the only collective
 * is the line-search cost reduction named by the design: one all-reduce of 8 doubles per iteration over RCCL/xGMI,
 *   vec8 = [ sum_b J_pred(alpha_1..6), sum_b delta_J, number of trajectories with a valid backward pass ]
 * summed over the trajectories of every rank whose status is 0.  Rank 0 creates the 128-byte RCCL unique id and the
 * host distributes it (file, pipe, MPI -- the library does no networking of its own); without kpilqr_comm_init the
 * call returns this rank's sums.  Enqueued on the context's stream after the forward pass; vec8 (host, may be NULL)
 * is valid after kpilqr_sync.  RCCL is loaded on first use (dlopen), not at link time. */
int  kpilqr_comm_unique_id(char id[128]);
int  kpilqr_comm_init(kpilqr_ctx *ctx, int nranks, int rank, const char id[128]);
int  kpilqr_allreduce_linesearch(kpilqr_ctx *ctx, double vec8[8]);

/* ---- debug / oracle hooks: inject or read the intermediates in the reference's layout -------
 * (the reference exposes A, B, l_x ... as public members, include/Optimiser/Optimiser.h:194-211,
 * and GenTestingData dumps them, src/GenTestingData.cpp:795-797).  NULL pointers are skipped. */
int  kpilqr_set_AB(kpilqr_ctx *ctx, const double *A, const double *B);
int  kpilqr_get_AB(kpilqr_ctx *ctx, double *A, double *B);
int  kpilqr_set_cost_derivs(kpilqr_ctx *ctx, const double *l_x, const double *l_xx,
                            const double *l_u, const double *l_uu);
int  kpilqr_get_cost_derivs(kpilqr_ctx *ctx, double *l_x, double *l_xx, double *l_u, double *l_uu);
/* The union of KPILQR_FLAG_UNION_KEYPOINTS, read back.  Both calls build it on demand (also for lists known to be uniform, whose
 * union is the list) and are synchronous; KPILQR_ERR_STATE when the flag is not active on this context (not set, or not a fused
 * one-tile shape) or there are no key-points yet.
 * kpilqr_get_union_keypoints: traj_offsets [batch+1] and ONE sorted list of union times per trajectory,
 * times[traj_offsets[b] .. traj_offsets[b+1]); times may be NULL to query the size.  Returns the total count or an error (< 0).
 * kpilqr_get_union_columns: the union column store [entry_u][3][n], entry_u = dof * traj_offsets[b] + d * |U_b| + j for
 * (trajectory b, DoF d, j-th union time), kinds as for kpilqr_upload_kp_columns; needs a resident FD payload
 * (KPILQR_ERR_STATE without one).  columns may be NULL to query the size.  Returns the number of union entries or an error. */
int  kpilqr_get_union_keypoints(kpilqr_ctx *ctx, int *traj_offsets /*[batch+1]*/, int *times, int times_capacity);
int  kpilqr_get_union_columns(kpilqr_ctx *ctx, double *columns, size_t capacity_doubles);

/* Name of the kernel variant the backward / forward pass will launch for these dims
 * ("mfma_f64_t1", "generic_lds", ...): for logs, tests and the bench's roofline line. */
const char *kpilqr_backward_variant(kpilqr_ctx *ctx);
const char *kpilqr_forward_variant(kpilqr_ctx *ctx);
/* What the LAST backward (which = 0) / forward (which = 1) launch of this context was -- the variant above and, for the
 * KPILQR_FLAG_FUSED sweeps, the form the library picked from the batch size, the payload and the key-point lists:
 *     "<variant>:<waves>:<columns>:<lists>[:ru0][:rxc][:slopes][:union]"  e.g. "mfma_f64_t1_fused:w1:raw:uni:ru0"
 *   waves    w1 one wavefront per trajectory | pair | triple | pairh (backward: consumer / helper pair)
 *            (forward `pair` on a uniform set: state wave with its own interpolant + scoring wave)
 *   columns  (backward only) raw: the sweep differenced the key-point ordered FD payload itself | kpc: it read the differenced
 *            key-point column store
 *   lists    uni: every DoF of a trajectory has the same key-point list (set_interval ...) | ragged: per-DoF lists
 *   ru0      no control residuals (r_u never uploaded): the products with r_u are left out
 *   rxc      constant residual Jacobians kept in registers (kpilqr_upload_residual_jacobians_const)
 *   slopes   per-DoF lists walked on precomputed segment slopes (a crossing is loads only)
 *   union    always last: the launch ran on the union store of KPILQR_FLAG_UNION_KEYPOINTS (`lists` is then the union's: uni),
 *            e.g. "mfma_f64_t1_fused:w1:kpc:uni:ru0:rxc:union"
 * The `lists` token is decided on the device; this call reads the flag back and therefore WAITS for the context's stream.
 * which = 2: the linearisation stage (differencing + interpolation of A, B) of the last kpilqr_fd_interpolate, kpilqr_iterate or
 * kpilqr_iterate_streamed; does not wait.  "" before any of them (and in a library without kpilqr_fd_interpolate), else
 *     "fd_kp_interpolate"          key-point ordered payload, one pass
 *     "kp_columns_interpolate"     column payload, one pass
 *     "fd_difference+interpolate"  the separate passes (job lists, or KPILQR_FD_INTERP=0)
 *     "in_sweep"                   KPILQR_FLAG_FUSED context: the sweeps difference and interpolate themselves
 *     "kp_union"                   the same on the union store of KPILQR_FLAG_UNION_KEYPOINTS (kpilqr_iterate with per-DoF lists)
 * with ":subset" appended when the last linearisation was a kpilqr_fd_interpolate_partial.
 * which = 3: how the last forward launch scored its steps (kpilqr_forward_linear[_partial], kpilqr_iterate[_partial] or the chunks of
 * kpilqr_iterate_streamed*); waits like which = 1.  "" before any forward launch and after a forward call that was refused before it
 * launched anything, else
 *     "pair2"   one residual-Jacobian product scores TWO steps: the one-wave sweep on uniform lists with the constant Jacobian
 *               ("...:w1:uni:ru0:rxc") and n_alpha <= 8 -- the candidates then fill at most half of the matrix tile's columns
 *     "step"    every step has its own product: every other launch
 *     "?"       the device's word on the key-point lists could not be read back (which = 1 then ends in ":?")
 *   A library older than this answer returns "" for which = 3 at all times; KPILQR_VERSION is unchanged.
 * For logs and tests (a test can assert which kernel form it exercised).  version >= 400. */
const char *kpilqr_last_launch(kpilqr_ctx *ctx, int which);

#ifdef __cplusplus
}
#endif
#endif
