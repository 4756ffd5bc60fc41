// common.h -- internal declarations shared by the translation units of libkpilqr.so.
// Not part of the public surface (that is include/kpilqr.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <type_traits>

#include "../../include/kpilqr.h"

namespace kpilqr {

// ---- device layout of one "step record" (all FP64), one per (trajectory b, time t) ----------
// [ A (n x n) | B (n x m) | l_xx (n x n) | l_x (n) | l_uu (m x m) | l_u (m) ].  A and B are COLUMN-major (as on the host):
// the finite differences produce COLUMNS, so k_fd_difference writes every job as one contiguous run of n doubles whatever
// the key-point pattern (with ragged per-DoF key-points a row-major record made every column n scattered 8-byte stores:
// n = 62, 26 % ragged key-points: 12.9 ms -> see DESIGN.md section 4.1), the interpolation walkers read contiguous
// runs, and the forward sweeps' A' operand is contiguous along lanes; the backward sweeps' tile loads become four
// consecutive rows (32 B) per lane quad.  l_xx and l_uu are symmetric, row-major.  Record stride is padded to 16 doubles
// (128 B).  a(row, col) / b(row, col): element offsets inside a record.
struct RecLayout {
    int n, m;
    int off_A, off_B, off_lxx, off_lx, off_luu, off_lu;
    int rec;      // used doubles
    int stride;   // padded stride in doubles
    __host__ __device__ RecLayout() {}
    __host__ __device__ RecLayout(int n_, int m_) : n(n_), m(m_) {
        off_A = 0;
        off_B = off_A + n * n;
        off_lxx = off_B + n * m;
        off_lx = off_lxx + n * n;
        off_luu = off_lx + n;
        off_lu = off_luu + m * m;
        rec = off_lu + m;
        stride = (rec + 15) & ~15;
    }
    __host__ __device__ int a(int row, int col) const { return off_A + col * n + row; }
    __host__ __device__ int b(int row, int col) const { return off_B + col * n + row; }
};

// ---- what one launch of a fused (one-tile) sweep is ------------------------------------------
// Made by plan_backward_fused / plan_forward_fused (fused_mfma.hip, where the policy is explained) and read by everyone else: the
// launchers map it to kernels, run_backward / run_forward ask it whether r_x needs its broadcast copy, kpilqr_last_launch prints it.
enum class Waves : int { none, w1, pair, triple, pairh };      // (kpilqr_last_launch's names; none: not a fused launch)
struct FusedLaunch {
    Waves waves = Waves::none;          // wave organisation: one wave per trajectory | state / cost pair | + staging wave | consumer / helper pair
    Waves waves_ragged = Waves::none;   // forward: what runs behind the uniform pair on per-DoF lists (triple or w1); else = waves
    bool raw = false;                   // backward: the sweep differences the key-point ordered payload itself
    bool ru0 = false;                   // r_u = 0: the instantiations without the r_u loads and the Ju product
    bool rxc = false;                   // constant r_x kept in registers (ru0 instantiations only): nobody reads the r_x buffer
    bool slopes = false;                // the general (per-DoF list) form walks the slope store
    bool excl = false;                  // w1: every wave has a SIMD to itself (EXCL instantiations)
    bool pair2 = false;                 // forward, w1 on uniform lists with rxc: one scoring product per two steps (n_alpha <= 8)
    bool fwd_ran = false;               // last_fwd only: the forward call that left this record launched its sweep (set behind the launch,
                                        // also on the empty record of a launch that is not fused); kpilqr_last_launch(ctx, 3) is "" without it
    bool uni_on_union = false;          // the launch ran on the union store (KPILQR_FLAG_UNION_KEYPOINTS); only kpilqr_last_launch reads it
};

// ---- device memory a context owns ------------------------------------------------------------
// Pointer and allocated bytes.  Trivially copyable and without a destructor on purpose: a view of a trajectory range
// (kpilqr_iterate_streamed) is a copy of the context with shifted pointers, and only kpilqr_destroy frees.  Sized by reserve()
// (kpilqr_api.cpp) and by nothing else; DevBuf<T> converts to T *, which is all the launchers see.
struct DevMem {
    void *p = nullptr;
    size_t cap = 0;               // allocated bytes
};
template <class T>
struct DevBuf : DevMem {
    operator T *() const { return static_cast<T *>(p); }
    void shift(size_t count) { p = static_cast<T *>(p) + count; }      // a view: count elements further on
};

// FD payload resident on the device: job lists (kpilqr_upload_fd / _slab) | one record per key-point entry (kpilqr_upload_fd_kp) |
// the differenced key-point columns themselves (kpilqr_upload_kp_columns: they live in kpc)
enum class FdPayload : int { none, jobs, kp_ordered, kp_columns };
// kernel family of a sweep, chosen per direction by select_variants (names: kpilqr_backward_variant)
enum class Family : int { generic, t1, tiled, wide, fused };

// ---- what is still valid ("Who says what is still valid") ---------------------------
// Two aggregates of Ctx, grouped by what their stores are derived from; an event resets an aggregate AS A WHOLE (= {}), so a flag
// added here later is cleared by construction.  A flag is set by the function that fills its store and by nobody else.
// From the resident FD payload and the key-point lists: reset by payload_changed (hence by keypoints_changed), size_buffers.
struct PayloadDerived {
    bool kpc_valid = false;      // kpc holds ALL differenced columns of the resident FD payload for the current key-points
    bool kpc_touched = false;    // a raw backward sweep has (re)written kpc from the resident payload since it was uploaded
    bool kps_valid = false;      // kps holds the slopes of the columns kpc holds (kpc_valid)
    bool kpcu_valid = false;     // kpcu is expanded from the current kpc
    bool rec_synced = false;     // the key-point columns of the resident payload (if any) are in the step records: set by the two functions
                                 // that write them for the whole batch (records_from_payload, linearise), a streamed iteration without a
                                 // new payload writes them first when it is clear.  NOT cleared by calls that overwrite records by hand
                                 // (set_AB, a record pointer, the A filter): such a sweep interpolates what they wrote
};
// From the key-point lists alone: reset by keypoints_changed, size_buffers.
struct ListsDerived {
    bool entry_tables_valid = false;     // kp_entry, kp_entry_list
    bool segent_valid = false;           // segent
    bool kpu_valid = false;              // the union lists (kpu_offsets, kpu_times, kpu_src, kpu_traj_first)
};

// ---- KPILQR_FLAG_EMBED_SHAPE: a one-tile shape without kernels of its own, zero-embedded into a compiled shape (its "carrier") --
// The context's own dims (Ctx::d, n, L, families, every launcher argument) are the CARRIER's; this holds the caller's and is looked at
// by the entry points of kpilqr_api.cpp and by the launchers of embed.hip alone -- no sweep kernel, launcher or launch plan sees it.
// State rows (and r_x columns) of the caller map to the carrier as i < dof -> i, i >= dof -> i + shift(carrier dof); controls are a
// prefix.  Padded states have zero A rows / columns, zero B rows and zero r_x columns, padded controls zero B columns.
struct Embed {
    bool on = false;
    int dof = 0, m = 0;           // the caller's
    int shift(int carrier_dof) const { return carrier_dof - dof; }
};

struct Ctx {
    kpilqr_dims d{};
    int n = 0;
    RecLayout L;
    hipStream_t stream = nullptr;
    int n_simd = 1024;             // SIMDs on the device (CUs x 4)
    bool own_stream = false;
    std::string err;
    PayloadDerived pay;
    ListsDerived lst;

    // device buffers (every DevBuf member is listed in for_each_buffer below; capacities are remembered, kpilqr_resize re-uses them)
    bool is_view = false;         // a copy made by make_view: it borrows the context's buffers and never allocates (reserve refuses)
    DevBuf<double> rec;           // [batch][T][stride]
    DevBuf<int> kp_uniform;       // device flag: every trajectory has one key-point list for all its DoFs (k_kp_uniform)
    DevBuf<double> K;             // [batch][T][n*m]
    DevBuf<double> k;             // [batch][T][m]
    DevBuf<float> K32;            // [count][T][n*m]: K of the trajectories of the last kpilqr_download_gains_f32[_partial], rounded to FP32 (gains.hip); reserved on demand
    DevBuf<double> r;             // [batch][T+1][nr]
    DevBuf<double> r_x;           // [batch][T+1][nr][n]
    DevBuf<double> r_u;           // [batch][T+1][nr][m]
    DevBuf<float> rj32;           // [r_x32 | r_u32]: the floats of the last kpilqr_upload_residual_jacobians_f32[_partial] on their way into r_x / r_u (residuals_f32.hip); reserved on demand
    DevBuf<double> w_run, w_term; // [nr]
    DevBuf<double> u_nom;         // [batch][T][m]
    DevBuf<double> ctrl_lim;      // [2m]
    DevBuf<double> lambda;        // [batch]
    DevBuf<double> alphas;        // [n_alpha]
    DevBuf<double> cost_pred;     // [batch][n_alpha]
    DevBuf<double> delta_J;       // [batch]
    DevBuf<double> traj_cost;     // [batch]
    DevBuf<int> status;           // [batch]
    // kpilqr_set_lambda_retry (lambda_retry.hip): sweeps each trajectory has run in the last backward pass under the schedule, and whether
    // the next attempt of the call in flight sweeps it again (1) or it is settled / has given up (0)
    DevBuf<int> attempts;         // [batch]
    DevBuf<int> gate;             // [batch]
    DevBuf<int> traj_list;        // [batch]: the trajectories of the partial record calls in flight (kpilqr_fd_interpolate_partial ...)
    DevBuf<int2> segmap;          // [batch][dof][T]: (start,end) key-points around t, or (-1,-1)
    // [batch][dof][T]: CSR entry of the key-point at or before t (the one-pass linearisation fetches a segment's endpoints by
    // entry), or -1 outside the list.  Built with segmap on a context that has records; on demand on a fused one (lst.segent_valid)
    DevBuf<int> segent;
    DevBuf<int> kp_offsets;       // [batch*dof+1]
    DevBuf<int> kp_times;         // [kp_total]
    bool have_kp = false;
    bool kp_canonical = false;   // every DoF list strictly increasing, first 0, last T-1 (what the fused sweeps walk)
    bool fused = false;          // KPILQR_FLAG_FUSED and a supported shape
    bool tiled_a6 = false;       // KPILQR_FLAG_FUSED on a tiled shape: the cost derivatives (a6) are formed inside the sweeps
    bool ru_zero = true;         // r_u was never written since create / resize (the buffer starts zeroed): r_u = 0 exactly
    // constant residual Jacobians (kpilqr_upload_residual_jacobians_const): ONE r_x [nr][n] for every trajectory and step.
    // rx_const_on: the fused one-wave sweeps keep it in registers and never read the r_x buffer; rx_buf_valid: the r_x buffer
    // holds the broadcast copy (made on demand for every other kernel family, ensure_rx_buffer)
    DevBuf<double> rx_const;
    bool rx_const_on = false, rx_buf_valid = true;
    bool rx_whole = false;       // every row of the r_x buffer has been given (a whole upload, the broadcast copy): rows of a subset may replace some

    // ---- fused contexts: the key-point column store (no step records) ---------------------------------------------------
    // A fused (one-tile) context does not allocate step records: its sweeps read the differenced key-point columns from
    //   kpc [entry][3][n],  entry = position in the per-DoF CSR (kp_offsets / kp_times),
    //                       kind 0: position column (A col d), 1: velocity column (A col d + dof), 2: control column (B col d, d < m)
    // i.e. 3n doubles per (trajectory, DoF, key-point) instead of a whole record per (trajectory, step).  The records are
    // allocated on demand when something asks for the materialised sequence (kpilqr_interpolate, get_AB, the error test ...).
    DevBuf<double> kpc;
    DevBuf<float> kpc32;          // [entries][3][n]: the encoded floats of the last kpilqr_upload_kp_columns_f32[_partial] or kp_columns32 of kpilqr_iterate_streamed3 on their way into kpc (columns_f32.hip); reserved on demand
    // slope store beside kpc (k_kp_slopes): kps [entry][3][n][2] = (column value, (column of the list's next key-point - this column) /
    // (time gap)) pairs, slope 0 for a list's last entry.  Read by the general (per-DoF list) forms of the one-wave sweeps; allocated only when the lists may be
    // ragged (kp_known_uniform: the host has seen that every trajectory's DoFs share one list -- then the device flag says the same
    // and only the segment-loop forms run)
    DevBuf<double> kps;
    bool kp_known_uniform = false;
    int kp_view_entries = -1;    // a view of a trajectory range: the CSR entries of its trajectories (first: fdk_first); -1: the context
    DevBuf<int> kp_entry;        // [batch*dof][T]: CSR entry of (list, t), or -1        (built with the segment map)
    DevBuf<int> kp_entry_list;   // [entries]: list (= b*dof + d) of a CSR entry
    bool have_rec = false;       // step records allocated (always on a non-fused context; on demand on a fused one)
    int kp_total_host = -1;      // number of CSR entries when the host knows it (kpilqr_set_keypoints), else -1
    int *kp_traj_first_host = nullptr;                // [batch+1] first CSR entry of every trajectory (host copy), or null
    FdPayload fd_payload = FdPayload::none;
    // key-point ordered payload: one record per CSR entry, [(x+, x-) pairs of the 3n elements | int32 mode, pad] = fdk_stride() bytes
    DevBuf<char> fdk_dev;
    size_t fdk_stride() const { return (size_t)(6 * n + 2) * 8; }
    int fdk_entries = 0;         // entries of the resident key-point ordered payload (a view: of its trajectories)
    int fdk_first = 0;           // first entry of a view's trajectories (0 for the context itself)

    // ---- KPILQR_FLAG_UNION_KEYPOINTS: per-DoF lists re-sampled onto their trajectory's union (kp_union.hip) ---------------------
    // Every DoF of trajectory b gets the union U_b of the trajectory's key-point times, so the lists are uniform and the
    // segment-loop forms of the sweeps run.  The union is stored once per DoF list, as an ordinary CSR the sweeps can read:
    //   kpu_offsets [batch*dof+1], kpu_offsets[b*dof+d] = dof * kpu_traj_first[b] + d * |U_b|;  kpu_times [dof * sum |U_b|]
    //   kpu_src [entry_u]: the own-list CSR entry p of the key-point at or before the union time; ~p when the time IS a key-point of the DoF
    //   kpcu [entry_u][3][n]: the union column store (k_kp_union_expand: copies and k_interpolate's interpolants of kpc)
    //   kpu_traj_first [batch+1]: union times before trajectory b (first the per-trajectory counts the host reads back and scans)
    DevBuf<int> kpu_offsets, kpu_times, kpu_src, kpu_traj_first;
    DevBuf<double> kpcu;
    DevBuf<int> kpu_uniform;     // the device flag a union view hands to the sweeps: always non-zero
    bool union_on = false;       // the flag is set and the context is fused (one-tile shape)
    int kpu_total = 0;           // sum over trajectories of |U_b| (entries_u = dof * kpu_total)
    int *kpu_traj_first_host = nullptr;               // [batch+1] host copy of kpu_traj_first

    // ---- kpilqr_update_keypoints: new lists for SOME trajectories, a by-entry payload carried over (kp_partial.hip) --------------
    // Second buffers of the payload slab, the column store and kp_times: the kept trajectories' records and lists are copied to
    // their new entry offsets in the second buffer, which is then SWAPPED with the live one (never in place: ranges move both ways).
    // Reserved the first time an update has something to carry, so the by-entry payload is held twice from then on.
    DevBuf<char> fdk_alt;
    DevBuf<double> kpc_alt;
    DevBuf<int> kp_times_alt;
    DevBuf<int> kp_upl_times;    // the new lists' times as uploaded
    DevBuf<int> kp_move;         // [3][batch+1]: first entry before | after | inside kp_upl_times (-1: kept), kp_merge_offsets
    // host mirrors (malloc): all offsets [batch*dof+1] (valid: filled by kpilqr_set_keypoints, read back once after
    // kpilqr_generate_keypoints) and per-trajectory flags [batch] (kp_merge.h) from which kp_canonical / kp_known_uniform follow
    int *kp_offsets_host = nullptr;
    bool kp_offsets_host_valid = false;
    unsigned char *kp_flags_host = nullptr;
    // the trajectories whose entry ranges wait for kpilqr_upload_fd_kp_partial / kpilqr_upload_kp_columns_partial: until then every
    // call that would read the payload is refused
    int *kp_pending_host = nullptr;       // [batch]
    int n_pending = 0, pending_entries = 0;

    // nominal states for on-device key-point placement (kpilqr_upload_states), allocated on first use
    DevBuf<double> X_states;      // [batch][T][n]
    DevBuf<double> kp_thr;        // [dof]
    DevBuf<unsigned long long> kp_mask;      // [batch*dof][ceil(T/64)]
    DevBuf<int> kp_count;         // [batch*dof]; kpilqr_generate_keypoints_partial: [2*batch*dof + 1], the compact counts | at batch*dof their scan
    bool have_states = false;
    // one host byte per trajectory (malloc, on first use): its states were given since create / resize -- by a whole
    // kpilqr_upload_states (everybody) or by kpilqr_upload_states_partial.  kpilqr_generate_keypoints_partial looks here.
    unsigned char *states_given_host = nullptr;      // [batch]

    // RCCL communicator for the line-search reduction (kpilqr_comm_init), and its 8-double device buffer
    void *comm = nullptr;
    int comm_ranks = 1;
    DevBuf<double> ls8;

    // FD job buffers: ONE device slab (grown on demand) whose layout mirrors the host slab of kpilqr_fd_slab_layout,
    // so that an upload is one hipMemcpyAsync; the pointers below point into it and are recomputed by every upload
    DevBuf<char> fd_dev;
    int njobs = 0, nnom = 0;
    int *job_b = nullptr, *job_t = nullptr, *job_col = nullptr, *job_nom = nullptr;
    unsigned char *job_mode = nullptr;
    double *xplus = nullptr, *xminus = nullptr, *xnom = nullptr;
    double eps = 1e-6;
    // a view of a trajectory range (kpilqr_iterate_streamed) has shifted per-trajectory pointers; the FD jobs carry
    // ABSOLUTE trajectory indices, so fd_difference addresses the records through the unshifted base
    double *rec_fd_base = nullptr;
    int fd_batch_total = 0;
    // device-side argument checks raise bits here; kpilqr_sync reads it back through the pinned mirror
    DevBuf<int> err_flag;
    int *err_flag_host = nullptr;          // pinned

    // trajectory-chunk pipeline of kpilqr_iterate_streamed: H2D(c+1) | kernels(c) | D2H(c-1) on separate streams
    // three streams: with the context's own stream that is the runtime's default of four hardware queues -- a fourth
    // chunk stream shares a queue with another one and the pipeline stalls (measured: B=256, resident Jacobians,
    // 22.7 ms with 3 chunks on 3 streams, 31.7 ms with 4 on 4; profiles/r02_pcie_inclusive.txt)
    static constexpr int kPipeStreams = 3;
    hipStream_t pipe_stream[kPipeStreams] = {nullptr, nullptr, nullptr};
    hipEvent_t pipe_done[kPipeStreams] = {nullptr, nullptr, nullptr};
    hipEvent_t pipe_in = nullptr;
    bool pipe_ready = false, pipe_dirty = false;
    int pipe_chunks = 0;
    unsigned long long pipe_sig = 0;       // hash of (njobs, nnom, traj_job_first, traj_nom_first) of the streamed iteration in flight
    // kpilqr_iterate_streamed2 with gain_traj: the list the chunks' gather launches read (gains.hip).  A device copy of its own -- not
    // traj_list, which the partial calls overwrite on the context's stream while chunks may still be reading -- and its pinned host
    // mirror: a call whose list equals the mirror uploads nothing and overlaps with the iteration in flight; a different list joins
    // the pipeline first (the rule of pipe_sig), and pipe_list_up says when the mirror may be overwritten (its upload has left it)
    DevBuf<int> pipe_list;                 // [batch], reserved by the first call that carries a list
    int *pipe_list_host = nullptr;         // [batch], pinned
    int pipe_list_count = -1;              // entries of the list pipe_list holds; -1: none yet
    hipEvent_t pipe_list_up = nullptr;
    // kpilqr_iterate_streamed4 with upload_traj (rows_in.hip).  rows_stage: one staging region per input kind, as large as the
    // whole-batch form of that input, reserved by the first call that gives the kind with a list and kept; a chunk uploads its compact
    // slice to where its first trajectory's rows (entries) would sit, so same-stream order protects the region from the next call's upload
    // whatever that call's list is.  (The FP32 columns stage in kpc32.)  The list changes with every iteration, so its device copy and
    // pinned mirror are a RING: slot rows_next holds [2][batch] ints -- the list | per trajectory the first entry of its payload inside
    // the staging region, -1: not listed.  A slot is written again kRowsRing calls later: the host then waits for the slot's own
    // upload (rows_up, long done), and the context's stream waits for the chunks that read the slot (rows_read), never for the
    // iteration in flight.
    enum RowsKind : int { kRowsR, kRowsRx, kRowsRu, kRowsUnom, kRowsPayload, kRowsKinds };
    DevBuf<char> rows_stage[kRowsKinds];
    static constexpr int kRowsRing = 4;
    DevBuf<int> rows_list;                 // [kRowsRing][2][batch]
    int *rows_list_host = nullptr;         // [kRowsRing][2][batch], pinned
    hipEvent_t rows_up[kRowsRing] = {};
    hipEvent_t rows_read[kRowsRing][kPipeStreams] = {};
    bool rows_read_set[kRowsRing][kPipeStreams] = {};
    int rows_next = 0;
    size_t rows_pay_rec = 0;               // bytes per entry of the payload last staged in rows_stage[kRowsPayload] (records | FP64 columns)
    // kpilqr_iterate_streamed5 with sweep_traj: the list the chunks' LISTED sweep launches, k_rows_in (the compact lambdas) and
    // k_rows_out (the compact small outputs) read.  The same ring scheme, [kRowsRing][batch] ints, reserved by the first call that
    // carries a non-empty sweep list and by nobody else.
    DevBuf<int> sweep_ring;                // [kRowsRing][batch]
    int *sweep_ring_host = nullptr;        // [kRowsRing][batch], pinned
    hipEvent_t sweep_up[kRowsRing] = {};
    hipEvent_t sweep_read[kRowsRing][kPipeStreams] = {};
    bool sweep_read_set[kRowsRing][kPipeStreams] = {};
    int sweep_next = 0;

    // ---- KPILQR_FLAG_EMBED_SHAPE (embed.hip) -------------------------------------------------------------------------------------
    // emb_stage: what crosses the link in the CALLER's shape, on its way in (payload, r_x, r_u, u_nom: one copy, then one embedding
    // launch) or out (K, k, U_alpha gathered by one launch, then one copy); reserved on demand, kept at the largest size asked for.
    // emb_offsets: the caller's CSR offsets [batch*dof + 1] on the device for the payload kernels; emb_offsets_host: their mirror.
    Embed embed;
    DevBuf<char> emb_stage;
    DevBuf<int> emb_offsets;
    int *emb_offsets_host = nullptr;      // [batch*dof + 1] (malloc), valid while have_kp
    int emb_entries = 0;                  // the caller's kp_offsets[batch*dof]

    // staging for debug hooks / U_alpha
    DevBuf<double> stage;
    // the compact host arrays of the listed sweeps (kpilqr_backward_partial, kpilqr_forward_linear_partial) on their way in and out:
    // [lambda | delta_J | cost_pred | status] of `count` rows; reserved by the first such call, never by anybody else
    DevBuf<char> sweep_stage;

    // everything the context owns on the device, once: kpilqr_destroy frees by walking this
    template <class F>
    void for_each_buffer(F f)
    {
        DevMem *const all[] = {&rec, &kp_uniform, &K, &k, &r, &r_x, &r_u, &w_run, &w_term, &u_nom, &ctrl_lim, &lambda, &alphas, &cost_pred,
                               &delta_J, &traj_cost, &status, &attempts, &gate, &traj_list, &K32, &segmap, &segent, &kp_offsets, &kp_times, &rx_const, &rj32, &kpc, &kpc32, &kps, &kp_entry,
                               &kp_entry_list, &fdk_dev, &kpu_offsets, &kpu_times, &kpu_src, &kpu_traj_first, &kpcu, &kpu_uniform, &fdk_alt, &kpc_alt, &kp_times_alt, &kp_upl_times, &kp_move, &X_states, &kp_thr, &kp_mask, &kp_count, &ls8, &fd_dev, &err_flag, &stage, &sweep_stage, &pipe_list,
                               &rows_stage[0], &rows_stage[1], &rows_stage[2], &rows_stage[3], &rows_stage[4], &rows_list, &sweep_ring, &emb_stage, &emb_offsets};
        for (DevMem *b : all) f(*b);
    }

    // The lambda retry schedule (kpilqr_set_lambda_retry; kept by kpilqr_resize).  retry_attempts: the attempts the backward pass about
    // to run launches, set by the entry point from the lambdas its caller passed.  bwd_gate: what the backward launchers look at -- nullptr
    // (GATED = false: the kernels of a context without a schedule) on the first attempt, `gate` on the attempts behind k_lambda_retry,
    // which launch the kernels' GATED instantiations.
    kpilqr_lambda_retry retry{};
    bool retry_on = false;
    bool retry_ran = false;       // a backward pass has run under the schedule since it was set: attempts holds its counts
    int retry_attempts = 1;
    const int *bwd_gate = nullptr;
    // A listed launch (kpilqr_backward_partial / kpilqr_forward_linear_partial): the device copy of the list (traj_list) in a copy of
    // the context whose d.batch is the list's length -- the launch width, by which the launchers choose their forms -- and whose
    // per-trajectory pointers stay the context's: block i sweeps trajectory sweep_list[i].  nullptr: every block sweeps its own index.
    // The backward launchers run a listed launch through the GATED instantiations, so it always comes with bwd_gate.
    const int *sweep_list = nullptr;

    Family bwd_family = Family::generic, fwd_family = Family::generic;
    // what the last backward / forward launch of this context actually was (kpilqr_last_launch); Waves::none: not a fused launch, or none yet
    FusedLaunch last_bwd, last_fwd;
    int last_width[2] = {-1, -1};      // trajectories of the last backward / forward launch when it was a listed one (its launch width), -1: the whole batch
    std::string launch_desc[2];
    const char *last_linearise = "";   // kpilqr_last_launch(ctx, 2): how the last linearisation (a2 + a4) ran

    // Diagnostic switches, read from the environment ONCE by kpilqr_create; the launchers only
    // look here.  0 = let the library choose.
    struct Tuning {
        int fused_bwd_waves = 0;   // KPILQR_FUSED_WAVES: 1 one wave, 5 consumer / helper pair (include/kpilqr.h lists every switch)
        int fused_fwd_waves = 0;   // KPILQR_FUSED_FWD_WAVES: 1 one wave, 3 triple, 4 pair with a form behind it for per-DoF lists
        int role_shift = 9;        // KPILQR_ROLE_SHIFT (wave-pair role placement probe)
        int tiled_nt_min = 0;      // KPILQR_TILED_NT_MIN: run the tiled kernels with more tiles than needed
        int tiled_a6 = -1;         // KPILQR_TILED_A6: -1 auto, 0 | 1
        int tiled_uw = -1;         // KPILQR_TILED_UW: 0 = no u-wave in the tiled backward sweep (NT <= 3, materialised tiles)
        int tiled_fsc = -1;        // KPILQR_TILED_FSC: -1 auto, 0 | 1: the state / cost wave groups of the two-tile forward sweep
        int fused_uni = -1;        // KPILQR_FUSED_UNI: 0 never take the uniform-key-point form of the one-wave backward sweep (diagnostic)
        int fused_raw = -1;        // KPILQR_FUSED_RAW: 0 never difference inside the backward sweep (diagnostic), else auto
        int fd_interp = -1;        // KPILQR_FD_INTERP: 0 = never difference and interpolate in one pass (the three-pass sequence runs), else auto
        int pipe_copy = -1;        // KPILQR_PIPE_COPY: chunk pipeline copies by kernel: bit 0 uploads, bit 1 downloads (-1 auto)
    } tune;
};

Ctx::Tuning read_tuning_from_env();

// The trajectory a block of a sweep works on: its own index, but in a listed launch (Ctx::sweep_list) entry blockIdx.x of the list --
// a scalar load off a kernel argument indexed by the block, so the index stays wave-uniform for the descriptors built from it.
__device__ __forceinline__ int kp_block_traj(const int *__restrict__ list, int own) { return list ? list[blockIdx.x] : own; }

// The sweep kernels' trailing template flags (backward `..., bool EXCL, bool GATED`, forward `..., bool EXCL,
// bool LISTED`) from the two runtime conditions that decide them: f is a generic lambda that names its instantiation with the two
// std::bool_constant it is given and launches it -- one launch, one argument list, whatever the flags.
template <class F>
inline auto kp_with_flags(bool first, bool second, F &&f)
{
    if (first) return second ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    return second ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

#define KP_HIP(ctx, call)                                                        \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) {                                                  \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);      \
            return KPILQR_ERR_HIP;                                               \
        }                                                                        \
    } while (0)

// ---- launchers (defined in the .hip files) --------------------------------------------------
// elementwise.hip
hipError_t launch_fd_difference(Ctx *c);                 // job lists -> step records
hipError_t launch_fd_difference_kpc(Ctx *c);             // job lists -> key-point column store
// key-point ordered payload -> key-point column store (only_if_ragged: leaves at once when the device flag kp_uniform is set;
// with_slopes: also the slope store of per-DoF lists, which the caller has sized for the current lists -- ensure_kps)
hipError_t launch_fd_kp_difference(Ctx *c, bool only_if_ragged = false, bool with_slopes = true);
hipError_t launch_kpc_to_records(Ctx *c, int first, int entries);   // key-point column store -> step records, CSR entries [first, first + entries)
hipError_t launch_kp_slopes(Ctx *c, bool only_if_ragged = true);   // key-point column store -> slope store (per-DoF lists only)
hipError_t launch_build_entry_tables(Ctx *c);            // kp_entry, kp_entry_list from the CSR lists
hipError_t launch_copy_out(hipStream_t s, double *dst_host, const double *src_dev, size_t count);   // D2H by a kernel
hipError_t launch_copy_in(hipStream_t s, void *dst_dev, const void *src_host, size_t bytes);        // H2D by a kernel
hipError_t launch_build_segmap(Ctx *c, bool segent_only = false);   // segmap (and segent when allocated); segent_only: segent alone
// kp_union.hip: the union of a trajectory's per-DoF key-point lists (KPILQR_FLAG_UNION_KEYPOINTS)
hipError_t launch_kp_union_count(Ctx *c);                // |U_b| of every trajectory -> kpu_traj_first [batch]
hipError_t launch_kp_union_build(Ctx *c);                // kpu_traj_first (scanned) -> kpu_offsets, kpu_times, kpu_src
hipError_t launch_kp_union_expand(Ctx *c);               // kpc -> kpcu
// kp_partial.hip: kpilqr_update_keypoints -- kept trajectories' records / lists to their new entry offsets in a second buffer
// (first_old, first_new, upl_first: the three rows of Ctx::kp_move; units: 16-byte units per record)
hipError_t launch_relocate_entries(Ctx *c, int units, long long longest_kept_entries, const int *first_old, const int *first_new,
                                   const int *upl_first, const void *src, void *dst);
hipError_t launch_merge_kp_times(Ctx *c, int longest_entries, const int *first_old, const int *first_new, const int *upl_first,
                                 const int *old_times, const int *upl_times, int *times);
// gains.hip: K of `count` trajectories (traj: their indices on the device; nullptr: trajectories 0 .. count-1) -> out [count][T][n][m], FP32
hipError_t launch_gains_f32(Ctx *c, const int *traj, int count, float *out);
// gains.hip, the chunks of kpilqr_iterate_streamed2: rows of the resident K or k gathered and stored straight into mapped pinned host
// memory on stream s.  Row i of `count` is trajectory traj[i] (device; nullptr: first + i) of the CONTEXT's buffers (c is never a view);
// dst [count][row] compact.  K_f32: K rounded to FP32 | K_f64, k_f64: as they are
enum class GainsForm : int { K_f32, K_f64, k_f64 };
hipError_t launch_gains_out(const Ctx *c, hipStream_t s, GainsForm form, const int *traj, int first, int count, void *dst_host);
// columns_f32.hip: the encoded FP32 key-point columns in src (device) decoded into the column store.  upl_first == nullptr: src holds
// every entry; else upl_first [batch] (device, the third row of Ctx::kp_move): first entry of a listed trajectory inside src, -1: not listed
hipError_t launch_kp_columns_f32(Ctx *c, const float *src, const int *upl_first);
// the same for a chunk of kpilqr_iterate_streamed3: the lists [l0, l1) = [b0*dof, b1*dof) of the CONTEXT's device CSR (c is never a view),
// decoded on stream s from `staging` (Ctx::kpc32, in store order: a list's floats sit at its first entry * 3n) into the column store
// upl_first != nullptr (a chunk of kpilqr_iterate_streamed4 with upload_traj): staging holds the chunk's LISTED trajectories' entries alone;
// upl_first [batch] (device): first entry of trajectory b inside staging, -1: not listed, its lists are left alone
hipError_t launch_kp_columns_f32_range(Ctx *c, hipStream_t s, int l0, int l1, const float *staging, const int *upl_first = nullptr);
// residuals_f32.hip: `count` trajectories of `per` floats each, compact in src (device; 8-byte aligned when per is even), widened into
// rows traj[i] (device; nullptr: rows 0 .. count-1) of dst, `per` doubles per trajectory, on the context's stream
hipError_t launch_widen_rows(Ctx *c, const int *traj, int count, long long per, const float *src, double *dst);
// the same for a chunk of kpilqr_iterate_streamed6, BOTH arrays in one launch on stream s: row i of `count` rows of src_x (perx floats
// a row) and src_u (peru floats a row) widened into trajectory traj[i] (device; nullptr: first + i) of dst_x / dst_u.  A NULL source
// is an array that is not given.  The sources may be device memory or the caller's pinned floats; src_x, and src_u when peru is even,
// 8-byte aligned
hipError_t launch_widen_jacobians(hipStream_t s, const int *traj, int first, int count, long long perx, const float *src_x, double *dst_x,
                                  long long peru, const float *src_u, double *dst_u);
// rows_in.hip, the chunks of kpilqr_iterate_streamed4 with upload_traj: rows of a chunk's staging region moved to their trajectories'
// places on stream s.  Row i of `count` is trajectory traj[i] (device).  Fixed rows of `units` doubles: staging + i*units -> dst + traj[i]*units
hipError_t launch_rows_in(hipStream_t s, const int *traj, int count, long long units, const double *staging, double *dst);
// rows by key-point entry (records of the key-point ordered payload, FP64 columns; rec_bytes per entry, a multiple of 16): the entry
// range of trajectory traj[i] in the CONTEXT's device CSR (c is never a view), read from entry src_first[traj[i]] of staging
// (src_first [batch], device) and written to the trajectory's own range of dst
hipError_t launch_rows_in_entries(const Ctx *c, hipStream_t s, const int *traj, int count, const int *src_first, size_t rec_bytes,
                                  const void *staging, void *dst);
// lambda_retry.hip: attempts = 1, gate = 1 for every trajectory | between two attempts: status -> lambda, attempts, gate
// (a listed launch, Ctx::sweep_list: thread i works on trajectory sweep_list[i] and nobody touches an unlisted trajectory's words)
hipError_t launch_lambda_retry_begin(Ctx *c);
hipError_t launch_lambda_retry(Ctx *c);
hipError_t launch_gate_arm(Ctx *c);                      // gate = 1 for the listed trajectories: a listed sweep without a schedule
// rows_in.hip, the mirror image of launch_rows_in for the small per-trajectory outputs of the listed sweeps (status, delta_J, cost_pred):
// `count` rows of `words` 4-byte words, row traj[i] (device) of src -> row i of staging.  The chunks of kpilqr_iterate_streamed5 pass
// the caller's mapped pinned rows for `staging` (the route of launch_gains_out: no staging buffer, no second DMA), and to
// launch_rows_in, for their few compact lambdas, the caller's pinned rows as its source.
hipError_t launch_rows_out(hipStream_t s, const int *traj, int count, int words, const void *src, void *staging);
// embed.hip (KPILQR_FLAG_EMBED_SHAPE; c->d is the carrier's shape, c->embed the caller's).  src / dst are device pointers.
// the caller's key-point ordered payload (records of 6n + 2 doubles by the caller's CSR, c->emb_offsets) -> the carrier's records in
// c->fdk_dev by the carrier's CSR (c->kp_offsets), every byte of every carrier record written
hipError_t launch_embed_fd_kp(Ctx *c, const void *src);
// the caller's key-point columns [entries][3][n] -> the carrier's column store c->kpc [entries'][3][n'], every element written
hipError_t launch_embed_kp_columns(Ctx *c, const double *src);
// rows of a matrix sequence: src [rows][cols] -> columns j < split at j, j >= split at j + shift of dst [rows][dst_cols]; nothing
// else of dst is written (its padding was zeroed with the buffer)
hipError_t launch_embed_rows(Ctx *c, long long rows, int cols, int dst_cols, int split, int shift, const double *src, double *dst);
// the inverse for the outputs: dst [count][rows][n][m] compact (FP64, or FP32 by the cast of k_gains_f32 when as_f32) gathered from
// src [count][rows][n'][m'], row i < split at i, i >= split at i + shift
hipError_t launch_extract_gains(Ctx *c, int count, long long rows, int n, int m, int src_n, int src_m, int split, int shift,
                                const double *src, void *dst, bool as_f32);
// comm.cpp (RCCL opened lazily) and the pack kernel of elementwise.hip
const char *comm_unique_id(char *id128);
const char *comm_init(Ctx *c, int nranks, int rank, const char *id128);
void comm_destroy(Ctx *c);
const char *comm_allreduce8(Ctx *c, double *dev8);
hipError_t launch_pack_linesearch(Ctx *c, double *dev8);
// keypoints.hip
hipError_t launch_generate_keypoints(Ctx *c, int method, int min_N, int max_N, double dt, const double *thr_dev,
                                     const double *X_dev, unsigned long long *mask_dev, int *count_dev);
// the placement of a listed subset (kpilqr_generate_keypoints_partial): pass 1 over list_dev [count] (device) into COMPACT mask /
// count rows, and -- once the host has scanned the counts -- pass 3 from those rows into times_dev by offsets_dev [count*dof + 1]
hipError_t launch_kp_flags_listed(Ctx *c, int count, const int *list_dev, int method, int min_N, int max_N, double dt,
                                  const double *thr_dev, const double *X_dev, unsigned long long *mask_dev, int *count_dev);
hipError_t launch_kp_fill_listed(Ctx *c, int count, const unsigned long long *mask_dev, const int *offsets_dev, int *times_dev);
hipError_t launch_kp_error_test(Ctx *c, int n_iv, const int *iv_dev, int min_N, double threshold, unsigned char *good_dev);
hipError_t launch_interpolate(Ctx *c, const int *traj = nullptr, int count = 0);      // traj (device): those trajectories alone
// linearise.hip: key-point ordered payload (FdPayload::kp_ordered) or column payload (kp_columns) -> every step record's [A|B], a2 + a4 in one pass
hipError_t launch_fd_kp_interpolate(Ctx *c, const int *traj = nullptr, int count = 0);
hipError_t launch_filter_dynamics(Ctx *c, int method, const double *coefs_dev, int ncoef);
hipError_t launch_dof_importance(Ctx *c, int sampling, double *sums_dev);
hipError_t launch_cost_derivs(Ctx *c, const int *traj = nullptr, int count = 0);
hipError_t launch_broadcast_rx(Ctx *c);                  // rx_const -> r_x [batch][T+1][nr][n]
hipError_t launch_broadcast(hipStream_t s, const double *src_dev, int len, double *dst_dev, size_t reps);   // dst [reps][len] = src [len]
hipError_t launch_trajectory_cost(Ctx *c);
// pack/unpack between the reference layout (column-major, separate arrays) and step records
hipError_t launch_pack_AB(Ctx *c, const double *A, const double *B);      // device staging -> records
hipError_t launch_unpack_AB(Ctx *c, double *A, double *B);
hipError_t launch_pack_cost(Ctx *c, const double *lx, const double *lxx, const double *lu, const double *luu);
hipError_t launch_unpack_cost(Ctx *c, double *lx, double *lxx, double *lu, double *luu);

// svr.hip: iLQR_SVR's singular-vector DoF importance over the resident gains.  svr_lane_form: the lane-per-step form (bit-identical
// with host/SVR.cpp) takes (n, m); svr_supported: some form does (the wave-per-step form keeps W in at most 64 KB of LDS).
bool svr_lane_form(int n, int m);
bool svr_supported(int n, int m);
size_t svr_stage_bytes(int batch, int dof, int m, int T, int sampling);     // work buffer of launch_dof_importance_svd
hipError_t launch_dof_importance_svd(Ctx *c, int sampling, double *work);   // sums [batch][dof] at the head of work

// riccati_generic.hip / forward_generic.hip: any (n, m); LDS-resident, op order of the reference.
hipError_t launch_backward_generic(Ctx *c, int pd_stride);
hipError_t launch_forward_generic(Ctx *c, double *U_alpha_dev);
size_t backward_generic_lds_bytes(int n, int m);

// riccati_mfma.hip / forward_mfma.hip: n+1 <= 16 and m <= 15 (one 16x16 f64 MFMA tile per block).
bool backward_mfma_supported(int n, int m);
hipError_t launch_backward_mfma(Ctx *c, int pd_stride);
bool forward_mfma_supported(int n, int m, int n_alpha);
hipError_t launch_forward_mfma(Ctx *c, double *U_alpha_dev);

// tiled_mfma.hip: n+2 <= 64 (NT x NT grids of 16x16 tiles in LDS), m in {1,7}
int tiled_tiles(int n, int nt_min);                       // tiles per side of the tiled kernels' state grid
bool backward_tiled_supported(int n, int m, int nt_min);
hipError_t launch_backward_tiled(Ctx *c, int pd_stride);
size_t backward_tiled_lds_bytes(int nt);
bool forward_tiled_supported(int n, int m, int n_alpha, int nt_min);
bool forward_tiled_sc_selected(const Ctx *c);             // the state / cost wave groups will run (two tiles, small batches)
hipError_t launch_forward_tiled(Ctx *c, double *U_alpha_dev);
// tiled_wide.hip: the same sweeps with the control block over up to two tiles (8 < m <= 32 backward, 16 < m <= 32 forward)
bool backward_wide_supported(int n, int m, int nt_min);
hipError_t launch_backward_wide(Ctx *c, int pd_stride);
bool forward_wide_supported(int n, int m, int n_alpha, int nt_min);
hipError_t launch_forward_wide(Ctx *c, double *U_alpha_dev);
// fused_mfma.hip: a4 + a6 evaluated inside the sweeps (n+2 <= 16)
bool fused_supported(int n, int m, int nr, int dof, int T, int n_alpha);
FusedLaunch plan_backward_fused(const Ctx *c, bool raw);     // raw: the sweep differences the key-point ordered payload itself
FusedLaunch plan_forward_fused(const Ctx *c);
hipError_t launch_backward_fused(Ctx *c, const FusedLaunch &p, int pd_stride);
hipError_t launch_backward_fused_pair(Ctx *c, const FusedLaunch &p, int pd_stride);     // Waves::pairh (fused_mfma.hip, part 2)
hipError_t launch_forward_fused(Ctx *c, const FusedLaunch &p, double *U_alpha_dev);
hipError_t launch_backward_fused_stats(Ctx *c, int pd_stride, int *hist_dev);

}  // namespace kpilqr
