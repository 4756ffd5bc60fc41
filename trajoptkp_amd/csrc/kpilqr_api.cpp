// kpilqr_api.cpp -- the C ABI of libkpilqr.so (include/kpilqr.h): context lifetime, pinned
// staging, uploads/downloads and kernel dispatch.  No CPU fallback lives here: without a HIP
// device kpilqr_create fails with KPILQR_ERR_NO_DEVICE.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "common.h"
#include "mfma_common.h"      // (host side only: kp_t1_shape, kp_t1_carrier)
#include "kp_merge.h"

using namespace kpilqr;

static thread_local std::string g_err;

struct kpilqr_ctx : public Ctx {};

static int set_err(kpilqr_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg;
    g_err = msg;
    return code;
}

// memory the DMA engines can read in place: an async copy from it never has to be waited for before the call returns
static bool is_pinned(const void *p)
{
    if (!p) return true;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

// an async copy from (or the launch behind one of) a pageable host array is complete before the caller has the array back
static int wait_unless_pinned(kpilqr_ctx *c, const void *host)
{
    if (!is_pinned(host)) KP_HIP(c, hipStreamSynchronize(c->stream));
    return KPILQR_OK;
}

// chunk streams of kpilqr_iterate_streamed -> the context's stream: everything enqueued by a streamed iteration is
// ordered before whatever the caller enqueues next
static int join_pipeline(kpilqr_ctx *c)
{
    if (!c->pipe_dirty) return KPILQR_OK;
    for (int i = 0; i < Ctx::kPipeStreams; i++) {
        KP_HIP(c, hipEventRecord(c->pipe_done[i], c->pipe_stream[i]));
        KP_HIP(c, hipStreamWaitEvent(c->stream, c->pipe_done[i], 0));
    }
    c->pipe_dirty = false;
    return KPILQR_OK;
}

// every enqueueing entry point: select the context's device (several contexts per host thread), join the chunk streams
#define KP_ENTER(c)                                                   \
    do {                                                              \
        KP_HIP(c, hipSetDevice((c)->d.device));                       \
        if ((c)->pipe_dirty) { int rcj_ = join_pipeline(c); if (rcj_) return rcj_; } \
    } while (0)

// ---- device memory: every allocation of a context is made here ------------------------------------------------------------
// What a growing buffer allocates beyond the bytes asked for: need / div + add (div 0: nothing), so that sizes which move a little
// from one call to the next -- the key-point lists of the adaptive methods -- do not re-allocate every time.
struct Slack { size_t div, add; };
static constexpr Slack kExact{0, 0};              // the dimension-sized buffers and the staging area
static constexpr Slack kQuarter{4, 4096};         // per key-point entry: column store, slope store
static constexpr Slack kEighth{8, 4096};          // the two FD slabs

static bool would_grow(const DevMem &b, size_t need) { return need > b.cap; }

static hipError_t release(DevMem &b)
{
    const hipError_t e = b.p ? hipFree(b.p) : hipSuccess;
    b = DevMem{};
    return e;
}

// how everything that allocates refuses a view of kpilqr_iterate_streamed's chunks
static const char *const kViewNeverAllocates = "a view of a trajectory range never allocates: its context sizes the buffers first";

// Room for `need` bytes in b.  Nothing happens while they fit; otherwise the old allocation is freed -- after a wait for the
// context's stream: nothing in flight still uses it -- and need + slack bytes are allocated.  Returns 1 when it re-allocated (the
// old contents are gone), 0 when not, an error code < 0.  zero: the `need` bytes are cleared, grown or not.
static int reserve(kpilqr_ctx *c, DevMem &b, size_t need, Slack slack, bool zero)
{
    int grown = 0;
    if (would_grow(b, need)) {
        if (c->is_view) return set_err(c, KPILQR_ERR_STATE, kViewNeverAllocates);
        if (b.p) KP_HIP(c, hipStreamSynchronize(c->stream));
        KP_HIP(c, release(b));
        const size_t bytes = need + (slack.div ? need / slack.div + slack.add : 0);
        const hipError_t e = hipMalloc(&b.p, bytes);
        if (e != hipSuccess) { b.p = nullptr; return set_err(c, KPILQR_ERR_ALLOC, std::string("hipMalloc failed: ") + hipGetErrorString(e)); }
        b.cap = bytes;
        grown = 1;
    }
    if (zero && need) KP_HIP(c, hipMemsetAsync(b.p, 0, need, c->stream));
    return grown;
}

// the staging area of the debug hooks / U_alpha
static int ensure_stage(kpilqr_ctx *c, size_t bytes)
{
    const int rc = reserve(c, c->stage, bytes, kExact, false);
    return rc < 0 ? rc : KPILQR_OK;
}

static int check_complete(kpilqr_ctx *c, const char *who);      // (below: ranges pending since kpilqr_update_keypoints)

// ---- KPILQR_FLAG_EMBED_SHAPE: the caller's shape at the ABI boundary (include/kpilqr.h, "Embedded shapes"; embed.hip) --------------
// c->d, c->n are the carrier's on an embedded context; these are what the caller's arrays are laid out by.
static int caller_dof(const kpilqr_ctx *c) { return c->embed.on ? c->embed.dof : c->d.dof; }
static int caller_n(const kpilqr_ctx *c) { return 2 * caller_dof(c); }
static int caller_m(const kpilqr_ctx *c) { return c->embed.on ? c->embed.m : c->d.m; }

// every entry point that is out of scope on an embedded context: refused first, before anything is enqueued or changed
static int refuse_embedded(kpilqr_ctx *c, const char *who)
{
    return set_err(c, KPILQR_ERR_STATE, std::string(who) + ": not on an embedded context (KPILQR_FLAG_EMBED_SHAPE: the call is out of scope there)");
}
#define KP_NOT_EMBEDDED(c, who) do { if ((c) && (c)->embed.on) return refuse_embedded((c), who); } while (0)

// the staging buffer of everything that crosses the link in the caller's shape; grows (after a stream sync) only when it has to
static int ensure_emb_stage(kpilqr_ctx *c, size_t bytes)
{
    const int rc = reserve(c, c->emb_stage, bytes, kEighth, false);
    return rc < 0 ? rc : KPILQR_OK;
}

// On an embedded context with padded controls (m' > m) the padded block of Q_uu + lambda I is lambda I: a lambda the host can see
// to be <= 0 (or NaN) would fail the first PD check of every trajectory for no reason of the caller's problem.  Refused before anything
// is enqueued; lambda = NULL (the resident lambdas) is accepted.
static int check_embedded_lambda(kpilqr_ctx *c, const char *who, const double *lambda)
{
    if (!c->embed.on || !lambda || c->d.m == c->embed.m) return KPILQR_OK;
    for (int b = 0; b < c->d.batch; b++)
        if (!(lambda[b] > 0.0))
            return set_err(c, KPILQR_ERR_ARG, std::string(who) + ": lambda[" + std::to_string(b) + "] is not > 0 on an embedded context with padded controls "
                           "(the padded block of Q_uu + lambda I is lambda I, which must be positive definite)");
    return KPILQR_OK;
}

static int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return (e && *e) ? atoi(e) : dflt;
}

namespace kpilqr {
Ctx::Tuning read_tuning_from_env()
{
    Ctx::Tuning t;
    t.fused_bwd_waves = env_int("KPILQR_FUSED_WAVES", 0);
    t.fused_fwd_waves = env_int("KPILQR_FUSED_FWD_WAVES", 0);
    t.role_shift = env_int("KPILQR_ROLE_SHIFT", 9);
    t.tiled_nt_min = env_int("KPILQR_TILED_NT_MIN", 0);
    t.tiled_a6 = env_int("KPILQR_TILED_A6", -1);
    t.tiled_uw = env_int("KPILQR_TILED_UW", -1);
    t.tiled_fsc = env_int("KPILQR_TILED_FSC", -1);
    t.pipe_copy = env_int("KPILQR_PIPE_COPY", -1);
    t.fused_raw = env_int("KPILQR_FUSED_RAW", -1);
    t.fused_uni = env_int("KPILQR_FUSED_UNI", -1);
    t.fd_interp = env_int("KPILQR_FD_INTERP", -1);
    return t;
}
}  // namespace kpilqr

// (Re)sizes every dimension-dependent device buffer of the context for c->d: a buffer is re-allocated only when it has to
// GROW (capacities are remembered), so shrinking the state vector and growing it back -- what iLQR_SVR does between
// optimisations -- re-uses the allocations.  Records, gains, residual and nominal-control buffers are zeroed.
static int size_buffers(kpilqr_ctx *c)
{
    const kpilqr_dims *dims = &c->d;
    c->n = 2 * dims->dof;
    c->L = RecLayout(c->n, dims->m);
    const size_t B = dims->batch, T = dims->T, n = c->n, m = dims->m, nr = dims->nr;
    const size_t segent_bytes = B * dims->dof * T * sizeof(int);
    // k_build_segmap writes segent wherever it exists: one a fused context built on demand must not outlive a shape it does not cover
    if (c->fused && would_grow(c->segent, segent_bytes)) KP_HIP(c, release(c->segent));
    c->pay = {}; c->lst = {};          // whatever was derived from the old shape's payload and lists
    struct Row { DevMem *buf; size_t bytes; bool zero; };      // zero: records start zeroed so that padding / never-written columns are defined
    const Row rows[] = {
        // a fused (one-tile) context keeps key-point columns only (Ctx::kpc); its records appear on demand (ensure_records)
        {&c->rec, c->fused ? 0 : B * T * c->L.stride * 8, true},
        {&c->K, B * T * n * m * 8, true},
        {&c->k, B * T * m * 8, true},
        {&c->r, B * (T + 1) * nr * 8, true},
        {&c->r_x, B * (T + 1) * nr * n * 8, true},
        {&c->r_u, B * (T + 1) * nr * m * 8, true},
        {&c->w_run, nr * 8, false},
        {&c->w_term, nr * 8, false},
        {&c->u_nom, B * T * m * 8, true},
        {&c->ctrl_lim, 2 * m * 8, false},
        {&c->lambda, B * 8, false},
        {&c->alphas, (size_t)dims->n_alpha * 8, false},
        {&c->cost_pred, B * dims->n_alpha * 8, false},
        {&c->delta_J, B * 8, false},
        {&c->traj_cost, B * 8, false},
        {&c->status, B * 4, true},
        {&c->attempts, B * 4, true},
        {&c->gate, B * 4, true},
        {&c->traj_list, B * sizeof(int), false},
        {&c->segmap, B * dims->dof * T * sizeof(int2), false},
        {&c->kp_offsets, (B * dims->dof + 1) * 4, false},
        // the entry map of the one-pass linearisation, beside segmap: with the records (a fused context builds it on demand, ensure_segent)
        {&c->segent, c->fused ? 0 : segent_bytes, false},
    };
    for (const Row &row : rows) {
        const int rc = reserve(c, *row.buf, row.bytes, kExact, row.zero);
        if (rc < 0) return rc;
    }
    c->have_rec = !c->fused;
    c->rec_fd_base = c->rec;
    c->fd_batch_total = dims->batch;
    return KPILQR_OK;
}

// ---- fused contexts: key-point column store, entry tables, records on demand ----------------------------------------------
// number of CSR entries of the current lists (known to the host since kpilqr_set_keypoints / kpilqr_generate_keypoints,
// which reads the total back); the capacity of kp_times before any key-points exist
static size_t kp_entries(const kpilqr_ctx *c)
{
    return c->kp_total_host >= 0 ? (size_t)c->kp_total_host : c->kp_times.cap / sizeof(int);
}

// a payload with one record (or three columns) per key-point entry: it is laid out BY the lists
static bool payload_by_entry(const kpilqr_ctx *c)
{
    return c->fd_payload == FdPayload::kp_ordered || c->fd_payload == FdPayload::kp_columns;
}

// kpc for the current key-points: 3n doubles per CSR entry (a quarter of slack, so that lists whose counts move a little
// from one linearisation to the next -- the adaptive methods -- do not re-allocate every time)
static int ensure_kpc(kpilqr_ctx *c)
{
    const size_t need = kp_entries(c) * 3 * (size_t)c->n * 8;
    const int rc = reserve(c, c->kpc, need, kQuarter, false);
    if (rc < 0) return rc;
    if (rc > 0) {              // a new store starts zeroed, slack included: entries come into use without passing through here
        KP_HIP(c, hipMemsetAsync(c->kpc, 0, c->kpc.cap, c->stream));
        const bool rec_synced = c->pay.rec_synced;           // (the records are not made from this store's bytes: they keep what they hold)
        c->pay = {};
        c->pay.rec_synced = rec_synced;
    }
    return KPILQR_OK;
}

// the slope store beside kpc, same size -- only when the lists may be per-DoF (ragged): uniform sets never read it
static int ensure_kps(kpilqr_ctx *c, bool force = false)
{
    if (c->kp_known_uniform && !force) return KPILQR_OK;
    const size_t need = kp_entries(c) * 6 * (size_t)c->n * 8;              // (value, slope) pairs
    const int rc = reserve(c, c->kps, need, kQuarter, false);
    if (rc < 0) return rc;
    if (rc > 0) c->pay.kps_valid = false;
    return KPILQR_OK;
}

// the slopes of the columns kpc holds (per-DoF lists: the general forms of the one-wave sweeps walk them; k_kp_slopes leaves at
// once when the device says the set is uniform).  always: whatever the lists and the flag say (kpilqr_backward_stats' general form)
static int slopes_for_kpc(kpilqr_ctx *c, bool always = false)
{
    if (!always && (c->pay.kps_valid || c->kp_known_uniform || !c->kps)) return KPILQR_OK;
    KP_HIP(c, launch_kp_slopes(c, !always));
    c->pay.kps_valid = true;
    return KPILQR_OK;
}

// kp_entry [list][t] and kp_entry_list [entry] for the current lists
static int ensure_entry_tables(kpilqr_ctx *c)
{
    if (c->lst.entry_tables_valid) return KPILQR_OK;
    int rc = reserve(c, c->kp_entry, (size_t)c->d.batch * c->d.dof * c->d.T * sizeof(int), kExact, false);
    if (rc < 0) return rc;
    rc = reserve(c, c->kp_entry_list, (kp_entries(c) ? kp_entries(c) : 1) * sizeof(int), Slack{4, 0}, false);
    if (rc < 0) return rc;
    KP_HIP(c, launch_build_entry_tables(c));
    c->lst.entry_tables_valid = true;
    return KPILQR_OK;
}

// The resident FD payload differenced into kpc (explicitly: the raw backward sweep does the same on the fly)
// want_slopes = false (the union route, whose sweeps never walk a slope store): none is allocated for it
static int difference_to_kpc(kpilqr_ctx *c, bool want_slopes = true)
{
    if (c->fd_payload == FdPayload::none || !c->have_kp) return KPILQR_OK;
    { const int rcp = check_complete(c, "differencing the resident payload"); if (rcp) return rcp; }      // (whoever asks: the entry points check first)
    if (c->fd_payload == FdPayload::kp_columns) {                       // the columns ARE the payload
        if (!c->pay.kpc_valid) return set_err(c, KPILQR_ERR_STATE, "the key-point columns are gone (new key-points): upload them again");
        return KPILQR_OK;
    }
    int rc = ensure_kpc(c);
    if (rc) return rc;
    // Only the fused sweeps' per-DoF list forms read the slope store, and only then is it sized for the current lists.  Anybody else
    // (the union route, a context with records) must not have it written: one that exists from earlier, shorter lists would be
    // written past its end.
    const bool slopes = c->fused && want_slopes;
    if (slopes) { rc = ensure_kps(c); if (rc) return rc; }
    c->pay.kps_valid = false;
    if (c->fd_payload == FdPayload::jobs) {
        rc = ensure_entry_tables(c);
        if (rc) return rc;
        KP_HIP(c, launch_fd_difference_kpc(c));
    } else {
        KP_HIP(c, launch_fd_kp_difference(c, false, slopes));
        if (slopes && c->kps && !c->kp_known_uniform) c->pay.kps_valid = true;         // (the slope store of per-DoF lists is written in the same pass)
    }
    c->pay.kpc_valid = true;
    return KPILQR_OK;
}

// The key-point columns of the resident FD payload written into the step records (what kpilqr_fd_difference means on a
// context that has records): the whole batch's (a view: its chunk's), and the one place besides linearise that says so
static int records_from_payload(kpilqr_ctx *c)
{
    if (c->fd_payload == FdPayload::jobs) KP_HIP(c, launch_fd_difference(c));
    else {
        { const int rcp = check_complete(c, "the records of the resident payload"); if (rcp) return rcp; }
        if (payload_by_entry(c) && c->have_kp) {
            int rc = KPILQR_OK;
            if (!c->pay.kpc_valid) rc = difference_to_kpc(c);
            if (rc) return rc;
            rc = ensure_entry_tables(c);
            if (rc) return rc;
            KP_HIP(c, launch_kpc_to_records(c, c->fdk_first, c->fdk_entries));
        }
    }
    c->pay.rec_synced = true;          // (no payload or no lists: nothing to write)
    return KPILQR_OK;
}

// segent for the current lists: built with segmap where the context has it allocated, else (a fused context) here
static int ensure_segent(kpilqr_ctx *c)
{
    if (c->lst.segent_valid) return KPILQR_OK;
    const int rc = reserve(c, c->segent, (size_t)c->d.batch * c->d.dof * c->d.T * sizeof(int), kExact, false);
    if (rc < 0) return rc;
    KP_HIP(c, launch_build_segmap(c, true));
    c->lst.segent_valid = true;
    return KPILQR_OK;
}

// The linearisation stage (a2 + a4) of a context that has records: [A|B] of every step from the resident payload.  A key-point
// ordered or column payload goes through k_fd_kp_interpolate (linearise.hip), one pass that leaves kpc alone -- kpc_valid /
// kpc_touched / kps_valid keep saying what kpc holds, so a later call that needs the column store differences the payload again;
// job lists, and everything under KPILQR_FD_INTERP=0, run the sequence difference -> kpc -> records -> k_interpolate.
static bool linearise_one_pass(const kpilqr_ctx *c)
{
    if (c->tune.fd_interp == 0) return false;
    if (c->fd_payload == FdPayload::kp_columns) return c->pay.kpc_valid;
    return c->fd_payload == FdPayload::kp_ordered;
}

// from_payload = false: the records hold the payload's key-point columns already (a chunk of a streamed iteration that brought
// no new payload), so k_interpolate alone runs and rec_synced is left as it is.
static int linearise(kpilqr_ctx *c, bool from_payload = true)
{
    if (from_payload && linearise_one_pass(c)) {
        const int rc = ensure_segent(c);
        if (rc) return rc;
        KP_HIP(c, launch_fd_kp_interpolate(c));
        c->last_linearise = c->fd_payload == FdPayload::kp_columns ? "kp_columns_interpolate" : "fd_kp_interpolate";
        c->pay.rec_synced = true;
        return KPILQR_OK;
    }
    if (from_payload) { const int rc = records_from_payload(c); if (rc) return rc; }
    KP_HIP(c, launch_interpolate(c));
    c->last_linearise = "fd_difference+interpolate";
    return KPILQR_OK;
}

// A fused context has no step records until something asks for the materialised sequence (kpilqr_interpolate, get_AB /
// set_AB, the cost-derivative hooks, the key-point error test, KPILQR_BUF_STEP_RECORDS): then they are allocated, zeroed
// and given the key-point columns of the resident payload.
static int ensure_record_storage(kpilqr_ctx *c)
{
    if (!c->have_rec) {
        const int rc = reserve(c, c->rec, (size_t)c->d.batch * c->d.T * c->L.stride * 8, kExact, true);
        if (rc < 0) return rc;
        c->rec_fd_base = c->rec;
        c->have_rec = true;
        c->pay.rec_synced = false;
    }
    return KPILQR_OK;
}

static int ensure_records(kpilqr_ctx *c)
{
    { const int rc = ensure_record_storage(c); if (rc) return rc; }
    return c->pay.rec_synced ? KPILQR_OK : records_from_payload(c);
}

// a new FD payload or new key-points: whatever was derived from the old ones is stale
static void payload_changed(kpilqr_ctx *c)
{
    c->pay = {};
    c->n_pending = c->pending_entries = 0;      // (a whole payload, new lists for everybody, or the partial upload that was waited for)
}

// kpilqr_update_keypoints has left entry ranges of the resident payload unwritten: nothing may read it before the partial upload
static int check_complete(kpilqr_ctx *c, const char *who)
{
    if (!c->n_pending) return KPILQR_OK;
    return set_err(c, KPILQR_ERR_STATE, std::string(who) + ": the payload of " + std::to_string(c->n_pending) + " trajectories (first: " +
                   std::to_string(c->kp_pending_host[0]) + ", " + std::to_string(c->pending_entries) + " entries) is pending since kpilqr_update_keypoints: "
                   "kpilqr_upload_fd_kp_partial / kpilqr_upload_kp_columns_partial is missing");
}

// ---- the calls on a subset of the batch (kpilqr_update_keypoints and the _partial family) ----------------------------------------
// What each of them does first, before anything is enqueued or changed: the argument check, KP_ENTER, and for `traj` [count]
//   listed          not through a view of a trajectory range; strictly increasing and within [0, batch)
//   listed_or_view  the list check alone (kpilqr_download_gains_partial reads through a view too; kpilqr_update_keypoints refuses
//                   one later, in the words of everything that allocates)
//   pending         nothing: the two payload uploads hold traj against the pending set (check_partial), and for them count = 0 is
//                   a call like any other while ranges are pending
// -> 1: go on | KPILQR_OK: nobody is listed, nothing to do | < 0: refused.  (They leave through wait_unless_pinned where a
// pageable array of the caller's is still being read.)
enum class Subset : int { listed, listed_or_view, pending };
static int enter_subset(kpilqr_ctx *c, const char *who, int count, const int *traj, Subset kind = Subset::listed)
{
    if (!c || count < 0 || (count > 0 && !traj)) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (kind == Subset::pending) return 1;
    if (count == 0) return KPILQR_OK;
    if (kind == Subset::listed && c->is_view) return set_err(c, KPILQR_ERR_STATE, std::string(who) + ": not through a view of a trajectory range");
    if (!kp_traj_list_ok(c->d.batch, count, traj)) return set_err(c, KPILQR_ERR_ARG, std::string(who) + ": traj must be strictly increasing and within [0, batch)");
    return 1;
}

// New key-point lists of `total` entries are on the device: everything that was derived from the old ones is stale, and a payload
// laid out by them is dropped (it has to follow them)
static void keypoints_changed(kpilqr_ctx *c, int total)
{
    c->kp_total_host = total;
    c->lst = {};
    if (payload_by_entry(c)) { c->fd_payload = FdPayload::none; c->fdk_entries = 0; }
    payload_changed(c);
}

// What kpilqr_set_keypoints, kpilqr_update_keypoints and kpilqr_generate_keypoints leave behind once the new lists (`total`
// entries) are enqueued on the device: the segment map, the event -- keypoints_changed FIRST, it resets the aggregate segent's
// mark lives in -- and then what is known about the new lists.  uniform: every trajectory's DoFs share one list.
static int lists_installed(kpilqr_ctx *c, int total, bool canonical, bool uniform)
{
    KP_HIP(c, launch_build_segmap(c));
    keypoints_changed(c, total);
    c->lst.segent_valid = c->segent != nullptr;          // (k_build_segmap writes segent wherever it exists)
    c->have_kp = true;
    c->kp_canonical = canonical;
    c->kp_known_uniform = uniform && c->tune.fused_uni != 0;      // (KPILQR_FUSED_UNI=0: the general forms run on every set)
    return KPILQR_OK;
}

// Host copy of the first CSR entry of every trajectory (kpilqr_iterate_streamed cuts an entry-ordered payload into chunks by it);
// false: no host memory
static bool remember_traj_first(kpilqr_ctx *c, const int *kp_offsets)
{
    if (!c->kp_traj_first_host) c->kp_traj_first_host = (int *)malloc(sizeof(int) * ((size_t)c->d.batch + 1));
    if (!c->kp_traj_first_host) return false;
    for (int b = 0; b <= c->d.batch; b++) c->kp_traj_first_host[b] = kp_offsets[(size_t)b * c->d.dof];
    return true;
}

// Host mirrors behind kpilqr_update_keypoints: the per-trajectory flags [batch] exist from the first key-points on; the offsets
// are copied here by kpilqr_set_keypoints (offs != null) or marked as to-be-read-back (kpilqr_generate_keypoints).  false: no memory
static bool remember_lists(kpilqr_ctx *c, const int *offs)
{
    const size_t nlists = (size_t)c->d.batch * c->d.dof;
    if (!c->kp_flags_host) c->kp_flags_host = (unsigned char *)malloc((size_t)c->d.batch);
    if (!c->kp_offsets_host) c->kp_offsets_host = (int *)malloc(sizeof(int) * (nlists + 1));
    if (!c->kp_flags_host || !c->kp_offsets_host) return false;
    if (offs) memcpy(c->kp_offsets_host, offs, sizeof(int) * (nlists + 1));
    c->kp_offsets_host_valid = offs != nullptr;
    return true;
}

static void forget_lists(kpilqr_ctx *c)
{
    int **const ints[] = {&c->kp_traj_first_host, &c->kp_offsets_host, &c->kp_pending_host};
    for (int **p : ints) { free(*p); *p = nullptr; }
    free(c->kp_flags_host); c->kp_flags_host = nullptr;
    c->kp_offsets_host_valid = false;
    c->n_pending = c->pending_entries = 0;
}

// Constant residual Jacobians (kpilqr_upload_residual_jacobians_const): a fused sweep whose plan says rxc keeps r_x in registers;
// every other sweep streams r_x per step from the context's buffer, which then receives the broadcast copy -- once, on demand.
static int ensure_rx_buffer(kpilqr_ctx *c)
{
    if (!c->rx_const_on || c->rx_buf_valid) return KPILQR_OK;
    KP_HIP(c, launch_broadcast_rx(c));
    c->rx_buf_valid = c->rx_whole = true;
    return KPILQR_OK;
}

// ---- KPILQR_FLAG_UNION_KEYPOINTS: per-DoF lists re-sampled onto their trajectory's union (kp_union.hip) ----------------------
// The sweeps of this launch take the union route: the flag is active, the lists are (or may be) per-DoF, and the uniform forms are
// not switched off.  Never through a view: kpilqr_iterate_streamed runs today's per-DoF forms chunk by chunk.
static bool union_route(const kpilqr_ctx *c)
{
    return c->union_on && !c->is_view && !c->kp_known_uniform && c->tune.fused_uni != 0;
}

// The union lists for the current key-points: the per-trajectory counts are read back (4 * batch bytes, ONE wait for the stream
// per key-point change), scanned on the host, and the buffers sized from the scan; a second launch writes the lists.
static int ensure_union(kpilqr_ctx *c)
{
    if (c->lst.kpu_valid) return KPILQR_OK;
    if (!c->kp_canonical)
        return set_err(c, KPILQR_ERR_STATE, "the key-point union needs canonical key-points (per DoF: strictly increasing, first 0, last T-1)");
    const size_t B = c->d.batch, dof = c->d.dof;
    int rc = reserve(c, c->kpu_traj_first, (B + 1) * sizeof(int), kQuarter, false);
    if (rc < 0) return rc;
    rc = reserve(c, c->kpu_offsets, (B * dof + 1) * sizeof(int), kQuarter, false);
    if (rc < 0) return rc;
    rc = reserve(c, c->kpu_uniform, sizeof(int), kQuarter, false);
    if (rc < 0) return rc;
    int *first = (int *)realloc(c->kpu_traj_first_host, sizeof(int) * (B + 1));
    if (!first) return set_err(c, KPILQR_ERR_ALLOC, "host allocation failed");
    c->kpu_traj_first_host = first;
    KP_HIP(c, launch_kp_union_count(c));
    KP_HIP(c, hipMemcpyAsync(first + 1, c->kpu_traj_first, B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    KP_HIP(c, hipStreamSynchronize(c->stream));
    first[0] = 0;
    for (size_t b = 0; b < B; b++) {
        const int cnt = first[b + 1];
        if (cnt < 2 || cnt > c->d.T || (size_t)first[b] + cnt > (size_t)INT32_MAX / dof)
            return set_err(c, KPILQR_ERR_HIP, "key-point union: implausible count read back");
        first[b + 1] = first[b] + cnt;
    }
    c->kpu_total = first[B];
    const size_t entries = dof * (size_t)c->kpu_total;
    rc = reserve(c, c->kpu_times, entries * sizeof(int), kQuarter, false);
    if (rc < 0) return rc;
    rc = reserve(c, c->kpu_src, entries * sizeof(int), kQuarter, false);
    if (rc < 0) return rc;
    // (the host array lives in the context and is rewritten only behind the wait above: a pageable source is safe)
    KP_HIP(c, hipMemcpyAsync(c->kpu_traj_first, first, (B + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, hipMemsetAsync(c->kpu_uniform, 1, sizeof(int), c->stream));          // any non-zero value: uniform
    KP_HIP(c, launch_kp_union_build(c));
    c->lst.kpu_valid = true;
    c->pay.kpcu_valid = false;
    return KPILQR_OK;
}

// kpcu expanded from what kpc holds (the caller has differenced the resident payload into it)
static int ensure_union_columns(kpilqr_ctx *c)
{
    int rc = ensure_union(c);
    if (rc) return rc;
    if (c->pay.kpcu_valid) return KPILQR_OK;
    rc = reserve(c, c->kpcu, (size_t)c->d.dof * c->kpu_total * 3 * c->n * 8, kQuarter, false);
    if (rc < 0) return rc;
    KP_HIP(c, launch_kp_union_expand(c));
    c->pay.kpcu_valid = c->pay.kpc_valid;          // (no payload: kpc is whatever it was left as, and is expanded again next time)
    return KPILQR_OK;
}

// kpc differenced from the resident payload (never by a raw sweep), the union built and expanded
static int prepare_union(kpilqr_ctx *c)
{
    int rc = ensure_kpc(c);
    if (rc) return rc;
    if (!c->pay.kpc_valid) { rc = difference_to_kpc(c, false); if (rc) return rc; }
    return ensure_union_columns(c);
}

// The context as the sweeps see it on the union route: a copy like make_view's (it never allocates) whose key-point lists and
// column store are the union's.  The lists are uniform by construction: only the segment-loop forms are launched, no slope
// store is needed, and nothing is differenced inside a sweep.  Status, delta_J, gains and costs land in the context's buffers.
static void make_union_view(const kpilqr_ctx *c, kpilqr_ctx *v)
{
    *v = *c;
    v->is_view = true;
    v->kp_offsets = c->kpu_offsets; v->kp_times = c->kpu_times; v->kp_uniform = c->kpu_uniform;
    v->kpc = c->kpcu; v->pay.kpc_valid = true;
    v->kps = DevBuf<double>{}; v->pay.kps_valid = false;
    v->kp_known_uniform = true;
    v->fd_payload = FdPayload::kp_columns;          // (nothing to difference: plan_backward_fused plans raw = false)
}

// what kpilqr_backward_variant / kpilqr_forward_variant call a family (a6: Ctx::tiled_a6)
static const char *variant_name(Family f, bool a6)
{
    switch (f) {
    case Family::t1: return "mfma_f64_t1";
    case Family::tiled: return a6 ? "mfma_f64_tiled_a6" : "mfma_f64_tiled";
    case Family::wide: return "mfma_f64_wide";
    case Family::fused: return "mfma_f64_t1_fused";
    case Family::generic: break;
    }
    return "generic_lds";
}

// kernel families for c->d
static int select_variants(kpilqr_ctx *c)
{
    const kpilqr_dims *dims = &c->d;
    c->fused = c->tiled_a6 = false;
    const bool generic = (dims->flags & KPILQR_FLAG_GENERIC_KERNELS) != 0;
    const bool force_tiled = (dims->flags & KPILQR_FLAG_TILED_KERNELS) != 0;
    c->bwd_family = (!generic && !force_tiled && backward_mfma_supported(c->n, dims->m)) ? Family::t1
                  : (!generic && backward_tiled_supported(c->n, dims->m, c->tune.tiled_nt_min)) ? Family::tiled
                  : (!generic && backward_wide_supported(c->n, dims->m, c->tune.tiled_nt_min)) ? Family::wide : Family::generic;
    c->fwd_family = (!generic && !force_tiled && forward_mfma_supported(c->n, dims->m, dims->n_alpha)) ? Family::t1
                  : (!generic && forward_tiled_supported(c->n, dims->m, dims->n_alpha, c->tune.tiled_nt_min)) ? Family::tiled
                  : (!generic && forward_wide_supported(c->n, dims->m, dims->n_alpha, c->tune.tiled_nt_min)) ? Family::wide : Family::generic;
    if ((dims->flags & KPILQR_FLAG_FUSED) && !generic && !force_tiled &&
        fused_supported(c->n, dims->m, dims->nr, dims->dof, dims->T, dims->n_alpha)) {
        c->fused = true;
        c->bwd_family = c->fwd_family = Family::fused;
    }
    c->union_on = c->fused && (dims->flags & KPILQR_FLAG_UNION_KEYPOINTS) != 0 && !c->embed.on;      // (ignored on any other shape, as FUSED is, and on an embedded context)
    // The same flag on a tiled shape (n + 2 > 16): a6 (variant "..._a6"), cost derivatives formed from the residuals inside the
    // sweeps.  It replaces k_cost_derivs (HBM-bound: n^2 doubles written per step) by NT*ceil(nr/4) + 6 MFMAs per wave-step of the
    // latency-bound backward sweep (+9 % at four tiles, whatever the batch): a gain from ~100 trajectories of a four-tile state up
    // (n = 62, B = 128, T = 5000: 74.4 -> 70.6 ms), a loss for two or three tiles at the batches measured.  KPILQR_TILED_A6 = 0 | 1.
    // (a4 inside the tiled sweeps existed in rounds 2-4, parity-green and slower by more than the k_interpolate it removed; removed
    // in round 5: tiled_mfma.hip.)
    if ((dims->flags & KPILQR_FLAG_FUSED) && c->bwd_family == Family::tiled && c->fwd_family == Family::tiled)
        c->tiled_a6 = dims->nr <= 16 && (c->tune.tiled_a6 >= 0 ? c->tune.tiled_a6 != 0
                                         : (tiled_tiles(c->n, c->tune.tiled_nt_min) == 4 && dims->batch >= 96));
    if (c->bwd_family == Family::generic && backward_generic_lds_bytes(c->n, dims->m) > 160 * 1024) {
        c->err = "state dimension too large for the generic backward kernel (LDS)";
        return KPILQR_ERR_ARG;
    }
    return KPILQR_OK;
}

// KPILQR_FLAG_EMBED_SHAPE: decided once, in kpilqr_create, before the families are selected.  The flag is ignored -- the way FUSED is on
// an unsupported shape -- without FUSED, with GENERIC or TILED forced, on a shape that has its own instantiation, and where no
// carrier exists (kp_t1_carrier; the fused sweeps' own bounds evaluated with the carrier's dims).  Otherwise the context's dims
// become the carrier's and c->embed keeps the caller's.
static void choose_embedding(kpilqr_ctx *c)
{
    const kpilqr_dims d = c->d;
    if (!(d.flags & KPILQR_FLAG_EMBED_SHAPE) || !(d.flags & KPILQR_FLAG_FUSED)) return;
    if (d.flags & (KPILQR_FLAG_GENERIC_KERNELS | KPILQR_FLAG_TILED_KERNELS)) return;
    if (kp_t1_shape(2 * d.dof, d.m)) return;
    int cdof = 0, cm = 0;
    if (!kp_t1_carrier(d.dof, d.m, &cdof, &cm)) return;
    if (!fused_supported(2 * cdof, cm, d.nr, cdof, d.T, d.n_alpha)) return;
    c->embed.on = true; c->embed.dof = d.dof; c->embed.m = d.m;
    c->d.dof = cdof; c->d.m = cm;
    c->n = 2 * cdof;
    c->L = RecLayout(c->n, cm);
}

extern "C" {

int kpilqr_version(void) { return KPILQR_VERSION; }

const char *kpilqr_strerror(kpilqr_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int kpilqr_create(const kpilqr_dims *dims, void *stream, kpilqr_ctx **out)
{
    if (!dims || !out) return set_err(nullptr, KPILQR_ERR_ARG, "null argument");
    *out = nullptr;
    if (dims->dof < 1 || dims->m < 1 || dims->T < 2 || dims->nr < 1 || dims->batch < 1 || dims->n_alpha < 1)
        return set_err(nullptr, KPILQR_ERR_ARG, "dims out of range");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return set_err(nullptr, KPILQR_ERR_NO_DEVICE,
                       std::string("no HIP device available (libkpilqr has no CPU fallback): ") +
                           (e != hipSuccess ? hipGetErrorString(e) : "device count 0"));
    if (dims->device < 0 || dims->device >= ndev) return set_err(nullptr, KPILQR_ERR_ARG, "device ordinal out of range");
    if (hipSetDevice(dims->device) != hipSuccess) return set_err(nullptr, KPILQR_ERR_NO_DEVICE, "hipSetDevice failed");

    kpilqr_ctx *c = new (std::nothrow) kpilqr_ctx();
    if (!c) return set_err(nullptr, KPILQR_ERR_ALLOC, "host allocation failed");
    c->tune = read_tuning_from_env();           // the only place the environment is looked at
    c->d = *dims;
    c->n = 2 * dims->dof;
    c->L = RecLayout(c->n, dims->m);
    choose_embedding(c);                        // (from here on c->d may be a carrier's shape; `dims` stays the caller's)
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dims->device) == hipSuccess && prop.multiProcessorCount > 0)
            c->n_simd = prop.multiProcessorCount * 4;
    }

    if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
            delete c; return set_err(nullptr, KPILQR_ERR_HIP, "hipStreamCreate failed");
        }
        c->own_stream = true;
    }

    {
        int rcs = select_variants(c);                        // first: a fused context allocates no step records
        if (rcs == KPILQR_OK) rcs = size_buffers(c);
        if (rcs >= 0) rcs = reserve(c, c->err_flag, sizeof(int), kExact, true);
        if (rcs >= 0) rcs = reserve(c, c->kp_uniform, sizeof(int), kExact, true);
        if (rcs >= 0) {
            const hipError_t e = hipHostMalloc((void **)&c->err_flag_host, sizeof(int), hipHostMallocDefault);
            if (e != hipSuccess) rcs = set_err(c, KPILQR_ERR_ALLOC, std::string("hipMalloc failed: ") + hipGetErrorString(e));
        }
        if (rcs < 0) { const std::string msg = c->err; kpilqr_destroy(c); return set_err(nullptr, rcs, msg); }
    }
    *out = c;
    return KPILQR_OK;
}

void kpilqr_destroy(kpilqr_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->d.device);
    (void)hipStreamSynchronize(c->stream);
    if (c->pipe_ready) {
        for (int i = 0; i < Ctx::kPipeStreams; i++) {
            if (c->pipe_stream[i]) { (void)hipStreamSynchronize(c->pipe_stream[i]); (void)hipStreamDestroy(c->pipe_stream[i]); }
            if (c->pipe_done[i]) (void)hipEventDestroy(c->pipe_done[i]);
        }
        if (c->pipe_in) (void)hipEventDestroy(c->pipe_in);
    }
    comm_destroy(c);
    c->for_each_buffer([](DevMem &b) { (void)release(b); });
    if (c->err_flag_host) (void)hipHostFree(c->err_flag_host);
    if (c->pipe_list_host) (void)hipHostFree(c->pipe_list_host);
    if (c->pipe_list_up) (void)hipEventDestroy(c->pipe_list_up);
    if (c->rows_list_host) (void)hipHostFree(c->rows_list_host);
    for (int i = 0; i < Ctx::kRowsRing; i++) {
        if (c->rows_up[i]) (void)hipEventDestroy(c->rows_up[i]);
        for (hipEvent_t e : c->rows_read[i]) if (e) (void)hipEventDestroy(e);
    }
    if (c->sweep_ring_host) (void)hipHostFree(c->sweep_ring_host);
    for (int i = 0; i < Ctx::kRowsRing; i++) {
        if (c->sweep_up[i]) (void)hipEventDestroy(c->sweep_up[i]);
        for (hipEvent_t e : c->sweep_read[i]) if (e) (void)hipEventDestroy(e);
    }
    forget_lists(c);
    free(c->states_given_host);
    free(c->emb_offsets_host);
    if (c->kpu_traj_first_host) free(c->kpu_traj_first_host);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int kpilqr_get_dims(kpilqr_ctx *c, kpilqr_dims *out)
{
    if (!c || !out) return KPILQR_ERR_ARG;
    *out = c->d;
    out->dof = caller_dof(c); out->m = caller_m(c);      // (an embedded context reports the caller's shape here)
    return KPILQR_OK;
}

// the shape the sweeps of an embedded context run at (KPILQR_FLAG_EMBED_SHAPE); KPILQR_ERR_STATE on a context that is not embedded
int kpilqr_get_carrier_dims(kpilqr_ctx *c, kpilqr_dims *out)
{
    if (!c || !out) return KPILQR_ERR_ARG;
    if (!c->embed.on) return set_err(c, KPILQR_ERR_STATE, "kpilqr_get_carrier_dims: the context is not embedded (KPILQR_FLAG_EMBED_SHAPE not set, or ignored for this shape)");
    *out = c->d;
    return KPILQR_OK;
}

// iLQR_SVR::Resize (src/Optimiser/iLQR_SVR.cpp:38-193): the optimiser changes the size of its state vector between
// optimisations.  Re-sizes the context in place; everything uploaded before (key-points, FD payload, residuals, nominal
// controls, weights, limits, alphas, lambda) is forgotten, the kernel families are re-selected.
int kpilqr_resize(kpilqr_ctx *c, int new_dof, int new_num_ctrl, int new_horizon)
{
    KP_NOT_EMBEDDED(c, "kpilqr_resize");
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (new_dof < 1 || new_num_ctrl < 1 || new_horizon < 2) return set_err(c, KPILQR_ERR_ARG, "dims out of range");
    KP_HIP(c, hipStreamSynchronize(c->stream));          // nothing in flight still uses the old layout
    const kpilqr_dims old = c->d;
    c->d.dof = new_dof; c->d.m = new_num_ctrl; c->d.T = new_horizon;
    c->n = 2 * new_dof; c->L = RecLayout(c->n, new_num_ctrl);
    int rc = select_variants(c);
    if (rc == KPILQR_OK) rc = size_buffers(c);
    if (rc != KPILQR_OK) {                              // leave a usable context behind
        const std::string msg = c->err;
        c->d = old;
        c->n = 2 * old.dof; c->L = RecLayout(c->n, old.m);
        (void)select_variants(c); (void)size_buffers(c);
        return set_err(c, rc, msg);
    }
    c->have_kp = c->kp_canonical = c->have_states = c->kp_known_uniform = false;
    free(c->states_given_host); c->states_given_host = nullptr;      // (nobody's states are given any more)
    c->njobs = c->nnom = 0;
    c->fd_payload = FdPayload::none; c->fdk_entries = 0; c->kp_total_host = -1;
    forget_lists(c);                                     // (sized by the old batch * dof; size_buffers has reset both validity aggregates)
    c->retry_ran = false;                                // (the lambda retry schedule itself stays; lambda and the counts are forgotten)
    c->ru_zero = true;                                   // size_buffers zeroed r_u
    c->rx_const_on = false; c->rx_buf_valid = true; c->rx_whole = false;
    // the key-point placement buffers were sized by the old shape: they are allocated again on first use
    DevMem *const placement[] = {&c->X_states, &c->kp_mask, &c->kp_count, &c->kp_thr};
    for (DevMem *b : placement) KP_HIP(c, release(*b));
    return KPILQR_OK;
}

int kpilqr_host_alloc(kpilqr_ctx *c, size_t bytes, void **pinned)
{
    if (!c || !pinned) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    KP_HIP(c, hipHostMalloc(pinned, bytes ? bytes : 1, hipHostMallocDefault));
    return KPILQR_OK;
}

int kpilqr_host_free(kpilqr_ctx *c, void *pinned)
{
    if (!c) {
        // the allocation may outlive the context it was made through (a binding whose arrays are still referenced after the
        // engine was closed): pinned host memory is not tied to a device or a stream
        if (pinned && hipHostFree(pinned) != hipSuccess) return set_err(nullptr, KPILQR_ERR_HIP, "hipHostFree failed");
        return KPILQR_OK;
    }
    KP_ENTER(c);
    if (pinned) KP_HIP(c, hipHostFree(pinned));
    return KPILQR_OK;
}

// Waits for the context's stream and reports what the device-side argument checks raised since the last report.  Used by
// kpilqr_sync and by every other entry point that synchronises (blocking downloads): a caller that never calls kpilqr_sync
// still sees a skipped FD job.
static int sync_and_report(kpilqr_ctx *c)
{
    KP_HIP(c, hipMemcpyAsync(c->err_flag_host, c->err_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    KP_HIP(c, hipStreamSynchronize(c->stream));
    if (*c->err_flag_host) {
        const int bits = *c->err_flag_host;
        KP_HIP(c, hipMemsetAsync(c->err_flag, 0, sizeof(int), c->stream));
        return set_err(c, KPILQR_ERR_ARG, (bits & 1) ? "FD job index out of range (trajectory, time, column, mode or nominal row): the job was skipped"
                                                     : "device-side argument check failed");
    }
    return KPILQR_OK;
}

int kpilqr_sync(kpilqr_ctx *c)
{
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    return sync_and_report(c);
}

int kpilqr_device_ptr(kpilqr_ctx *c, int which, void **dptr, size_t *bytes)
{
    if (!c || !dptr) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    // (an embedded context: the buffers laid out by the carrier's shape stay inside; the shape-free ones are the caller's as they are)
    if (c->embed.on && which != KPILQR_BUF_RESIDUALS && which != KPILQR_BUF_COST_PRED && which != KPILQR_BUF_DELTA_J && which != KPILQR_BUF_STATUS)
        return refuse_embedded(c, "kpilqr_device_ptr of a shape-dependent buffer");
    const size_t B = c->d.batch, T = c->d.T, n = c->n, m = c->d.m, nr = c->d.nr;
    void *p = nullptr; size_t sz = 0;
    switch (which) {
    case KPILQR_BUF_STEP_RECORDS: { const int rcr = ensure_records(c); if (rcr) return rcr; } p = c->rec; sz = B * T * c->L.stride * 8; break;
    case KPILQR_BUF_K: p = c->K; sz = B * T * n * m * 8; break;
    case KPILQR_BUF_k: p = c->k; sz = B * T * m * 8; break;
    case KPILQR_BUF_RESIDUALS: p = c->r; sz = B * (T + 1) * nr * 8; break;
    case KPILQR_BUF_R_X:
        // a writable pointer leaves the library: the buffer gets the constant Jacobians' broadcast copy and is what the
        // sweeps read from here on (the constant mode is off, as for r_u below)
        { const int rcx = ensure_rx_buffer(c); if (rcx) return rcx; }
        c->rx_const_on = false; c->rx_buf_valid = c->rx_whole = true;
        p = c->r_x; sz = B * (T + 1) * nr * n * 8; break;
    case KPILQR_BUF_R_U:
        // a writable pointer leaves the library: from here on r_u may be non-zero without kpilqr_upload_residuals having
        // seen it, so the r_u-free instantiations of the fused sweeps (Ctx::ru_zero) are off for this context
        p = c->r_u; sz = B * (T + 1) * nr * m * 8; c->ru_zero = false; break;
    case KPILQR_BUF_U_NOM: p = c->u_nom; sz = B * T * m * 8; break;
    case KPILQR_BUF_FD_XPLUS: p = c->xplus; sz = (size_t)c->njobs * n * 8; break;
    case KPILQR_BUF_FD_XMINUS: p = c->xminus; sz = (size_t)c->njobs * n * 8; break;
    case KPILQR_BUF_COST_PRED: p = c->cost_pred; sz = B * c->d.n_alpha * 8; break;
    case KPILQR_BUF_DELTA_J: p = c->delta_J; sz = B * 8; break;
    case KPILQR_BUF_STATUS: p = c->status; sz = B * 4; break;
    default: return set_err(c, KPILQR_ERR_ARG, "unknown buffer id");
    }
    *dptr = p;
    if (bytes) *bytes = sz;
    return KPILQR_OK;
}

// ---- STEP 1b ------------------------------------------------------------------------------------
static int install_lists(kpilqr_ctx *c, const int *kp_offsets, const int *kp_times);

// kpilqr_set_keypoints on an embedded context: the caller's lists are checked as they are, expanded on the host to the carrier's CSR
// (batch * dof' lists: the caller's lists d < dof, then dof' - dof COPIES of the trajectory's list 0 -- a trajectory whose lists
// are all equal stays uniform, so the segment-loop forms of the sweeps keep running) and installed through the one path.  The
// caller's offsets stay behind as a host mirror and a device copy: the payload kernels of embed.hip read records by them.
static int install_embedded_lists(kpilqr_ctx *c, const int *kp_offsets, const int *kp_times)
{
    const int B = c->d.batch, dof = c->embed.dof, cdof = c->d.dof;
    const size_t nlists = (size_t)B * dof;
    if (const char *bad = kp_check_lists(nlists, c->d.T, kp_offsets, kp_times)) return set_err(c, KPILQR_ERR_ARG, bad);
    std::vector<int> offs, times;
    offs.reserve((size_t)B * cdof + 1);
    offs.push_back(0);
    for (int b = 0; b < B; b++)
        for (int d = 0; d < cdof; d++) {
            const size_t l = (size_t)b * dof + (d < dof ? d : 0);
            times.insert(times.end(), kp_times + kp_offsets[l], kp_times + kp_offsets[l + 1]);
            if (times.size() > (size_t)INT32_MAX) return set_err(c, KPILQR_ERR_ARG, "kpilqr_set_keypoints: the expanded lists of the carrier shape exceed 2^31 entries");
            offs.push_back((int)times.size());
        }
    if (times.empty()) times.push_back(0);               // (a pointer to hand on; no entry is read)
    { const int rcg = reserve(c, c->emb_offsets, (nlists + 1) * sizeof(int), kExact, false); if (rcg < 0) return rcg; }
    if (!c->emb_offsets_host) c->emb_offsets_host = (int *)malloc(sizeof(int) * (nlists + 1));
    if (!c->emb_offsets_host) return set_err(c, KPILQR_ERR_ALLOC, "host allocation failed");
    // (the expanded arrays are pageable: the install path waits for their copies before it returns)
    { const int rc = install_lists(c, offs.data(), times.data()); if (rc) return rc; }
    memcpy(c->emb_offsets_host, kp_offsets, sizeof(int) * (nlists + 1));
    c->emb_entries = kp_offsets[nlists];
    KP_HIP(c, hipMemcpyAsync(c->emb_offsets, c->emb_offsets_host, (nlists + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    return KPILQR_OK;
}

int kpilqr_set_keypoints(kpilqr_ctx *c, const int *kp_offsets, const int *kp_times)
{
    if (!c || !kp_offsets || !kp_times) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    return c->embed.on ? install_embedded_lists(c, kp_offsets, kp_times) : install_lists(c, kp_offsets, kp_times);
}

static int install_lists(kpilqr_ctx *c, const int *kp_offsets, const int *kp_times)
{
    const size_t nlists = (size_t)c->d.batch * c->d.dof;
    if (const char *bad = kp_check_lists(nlists, c->d.T, kp_offsets, kp_times)) return set_err(c, KPILQR_ERR_ARG, bad);
    const int total = kp_offsets[nlists];
    { const int rcg = reserve(c, c->kp_times, (size_t)total * sizeof(int), Slack{4, 64 * sizeof(int)}, false); if (rcg < 0) return rcg; }
    if (!remember_lists(c, kp_offsets)) return set_err(c, KPILQR_ERR_ALLOC, "host allocation failed");
    // per trajectory (kpilqr_update_keypoints merges them): canonical lists; every DoF shares one list (set_interval) -- when that
    // holds for the whole batch the device flag of k_kp_uniform will say the same, only the segment-loop forms of the sweeps run
    // and no slope store is needed
    for (int b = 0; b < c->d.batch; b++) c->kp_flags_host[b] = kp_traj_flags(c->d.dof, c->d.T, kp_offsets + (size_t)b * c->d.dof, kp_times);
    const unsigned char flags = kp_batch_flags(c->d.batch, c->kp_flags_host);
    KP_HIP(c, hipMemcpyAsync(c->kp_offsets, kp_offsets, (nlists + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, hipMemcpyAsync(c->kp_times, kp_times, (size_t)total * sizeof(int), hipMemcpyHostToDevice, c->stream));
    { const int rci = lists_installed(c, total, flags & kKpCanonical, flags & kKpUniform); if (rci) return rci; }
    // pageable host arrays: make the copies complete before returning control (pinned ones are read in place)
    if (!(is_pinned(kp_offsets) && is_pinned(kp_times))) KP_HIP(c, hipStreamSynchronize(c->stream));
    if (!remember_traj_first(c, kp_offsets)) return set_err(c, KPILQR_ERR_ALLOC, "host allocation failed");
    return KPILQR_OK;
}

// ---- new lists for SOME trajectories: a payload laid out by entry follows them on the device (kp_partial.hip) ---------------------
// The batch offsets as the host knows them: kpilqr_set_keypoints left them; behind kpilqr_generate_keypoints they are read back
// here, once (a wait for the stream)
static int ensure_offsets_mirror(kpilqr_ctx *c)
{
    if (!c->kp_offsets_host || !c->kp_flags_host) return set_err(c, KPILQR_ERR_STATE, "kpilqr_update_keypoints: the context has no key-point lists yet");
    if (c->kp_offsets_host_valid) return KPILQR_OK;
    const size_t nlists = (size_t)c->d.batch * c->d.dof;
    KP_HIP(c, hipMemcpyAsync(c->kp_offsets_host, c->kp_offsets, (nlists + 1) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    KP_HIP(c, hipStreamSynchronize(c->stream));
    bool ok = c->kp_offsets_host[0] == 0 && c->kp_offsets_host[nlists] == c->kp_total_host;
    for (size_t i = 0; i < nlists && ok; i++) ok = c->kp_offsets_host[i + 1] >= c->kp_offsets_host[i];
    if (!ok) return set_err(c, KPILQR_ERR_HIP, "kpilqr_update_keypoints: implausible key-point offsets read back");
    c->kp_offsets_host_valid = true;
    return KPILQR_OK;
}

// What kpilqr_update_keypoints and kpilqr_generate_keypoints_partial share once the new lists of the `count` trajectories in `traj`
// are known (kp_offsets [count*dof + 1] from 0, on the host) and the context's offsets mirror is valid: the merge, the second
// buffers, the enqueue and the bookkeeping.  The two callers differ in where the new lists' TIMES are: kp_times != nullptr is the
// caller's host array, which goes up into kp_upl_times here and from which the listed trajectories' flags are taken; nullptr says
// that kp_upl_times (reserved by the caller for kp_offsets[count*dof] entries) already holds them on the device, placed there by
// k_kp_fill on the context's stream, and placed_flags is every listed trajectory's flag byte.
static int install_subset_lists(kpilqr_ctx *c, const char *who, int count, const int *traj, const int *kp_offsets, const int *kp_times,
                                unsigned char placed_flags)
{
    const int B = c->d.batch, dof = c->d.dof;
    const size_t nlists = (size_t)B * dof, nnew = (size_t)count * dof, B1 = (size_t)B + 1;
    int rc;
    // ---- the merged CSR and who moves where (kp_merge.h); nothing of the context changes before every buffer is there ------------
    int *merged = (int *)malloc(sizeof(int) * (nlists + 1)), *mv = (int *)malloc(sizeof(int) * 3 * B1);
    struct Free { int *a, *b; ~Free() { free(a); free(b); } } guard{merged, mv};
    if (!merged || !mv) return set_err(c, KPILQR_ERR_ALLOC, "host allocation failed");
    int *const first_old = mv, *const first_new = mv + B1, *const upl_first = mv + 2 * B1;
    if (!kp_merge_offsets(B, dof, c->kp_offsets_host, count, traj, kp_offsets, merged, first_old, first_new, upl_first))
        return set_err(c, KPILQR_ERR_ARG, std::string(who) + ": more key-point entries than an int counts");
    const int total = merged[nlists], new_entries = kp_offsets[nnew];
    int longest = 0, longest_kept = 0;
    for (int b = 0; b < B; b++) {
        if (first_new[b + 1] - first_new[b] > longest) longest = first_new[b + 1] - first_new[b];
        if (upl_first[b] < 0 && first_old[b + 1] - first_old[b] > longest_kept) longest_kept = first_old[b + 1] - first_old[b];
    }
    // a payload laid out by entry survives: the records of everybody who is not listed move to their new offsets.  Job lists carry
    // their own indices and stay as they are; without a payload there is nothing to carry.
    const FdPayload kind = c->fd_payload;
    const bool carry = kind == FdPayload::kp_ordered || (kind == FdPayload::kp_columns && c->pay.kpc_valid);
    DevMem *live = nullptr, *alt = nullptr;
    size_t rec_bytes = 0;
    if (kind == FdPayload::kp_ordered) { live = &c->fdk_dev; alt = &c->fdk_alt; rec_bytes = c->fdk_stride(); }
    else { live = &c->kpc; alt = &c->kpc_alt; rec_bytes = (size_t)3 * c->n * 8; }
    // Growth: the destinations are reserved FIRST (what reserve() frees is an old second buffer nobody reads any more), the copies
    // read the live buffers, and only the swap retires those -- to become the second buffers of the next update
    rc = reserve(c, c->kp_times_alt, (size_t)total * sizeof(int), Slack{4, 64 * sizeof(int)}, false);
    if (rc < 0) return rc;
    rc = reserve(c, c->kp_upl_times, (size_t)new_entries * sizeof(int), kQuarter, false);
    if (rc < 0) return rc;
    rc = reserve(c, c->kp_move, 3 * B1 * sizeof(int), kExact, false);
    if (rc < 0) return rc;
    if (carry) {
        rc = reserve(c, *alt, (size_t)total * rec_bytes, kQuarter, false);
        if (rc < 0) return rc;
        // (a new column store starts zeroed, slack included, as ensure_kpc's does)
        if (rc > 0 && kind == FdPayload::kp_columns) KP_HIP(c, hipMemsetAsync(alt->p, 0, alt->cap, c->stream));
    }

    // ---- enqueue: offsets and the move table up, lists merged, kept records moved, buffers swapped --------------------------------
    const int *const mv_dev = c->kp_move;
    KP_HIP(c, hipMemcpyAsync(c->kp_offsets, merged, (nlists + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, hipMemcpyAsync(c->kp_move, mv, 3 * B1 * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (new_entries && kp_times) KP_HIP(c, hipMemcpyAsync(c->kp_upl_times, kp_times, (size_t)new_entries * sizeof(int), hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, launch_merge_kp_times(c, longest, mv_dev, mv_dev + B1, mv_dev + 2 * B1, c->kp_times, c->kp_upl_times, c->kp_times_alt));
    std::swap(c->kp_times, c->kp_times_alt);
    if (carry) {
        KP_HIP(c, launch_relocate_entries(c, (int)(rec_bytes / 16), longest_kept, mv_dev, mv_dev + B1, mv_dev + 2 * B1, live->p, alt->p));
        std::swap(*live, *alt);
    }
    // ---- the context as kpilqr_set_keypoints(merged lists) leaves it -- except that the payload stays, with ranges pending ---------
    for (int i = 0; i < count; i++) c->kp_flags_host[traj[i]] = kp_times ? kp_traj_flags(dof, c->d.T, kp_offsets + (size_t)i * dof, kp_times) : placed_flags;
    const unsigned char flags = kp_batch_flags(B, c->kp_flags_host);
    rc = lists_installed(c, total, flags & kKpCanonical, flags & kKpUniform);
    if (rc) return rc;
    // the staging arrays above are this call's own: they are read before it returns
    KP_HIP(c, hipStreamSynchronize(c->stream));
    free(c->kp_offsets_host);
    c->kp_offsets_host = merged; guard.a = nullptr;
    if (!remember_traj_first(c, merged)) return set_err(c, KPILQR_ERR_ALLOC, "host allocation failed");
    if (carry) {
        if (!c->kp_pending_host) c->kp_pending_host = (int *)malloc(sizeof(int) * (size_t)B);
        if (!c->kp_pending_host) return set_err(c, KPILQR_ERR_ALLOC, "host allocation failed");      // (the payload is dropped: as kpilqr_set_keypoints)
        c->fd_payload = kind; c->fdk_entries = total; c->fdk_first = 0;
        memcpy(c->kp_pending_host, traj, sizeof(int) * (size_t)count);
        c->n_pending = count; c->pending_entries = new_entries;
    }
    return KPILQR_OK;
}

int kpilqr_update_keypoints(kpilqr_ctx *c, int count, const int *traj, const int *kp_offsets, const int *kp_times)
{
    KP_NOT_EMBEDDED(c, "kpilqr_update_keypoints");
    if (count > 0 && (!kp_offsets || !kp_times)) return KPILQR_ERR_ARG;
    // (count = 0: nobody's lists change, nothing becomes invalid; a view is refused below, in the words of everything that allocates)
    { const int go = enter_subset(c, "kpilqr_update_keypoints", count, traj, Subset::listed_or_view); if (go <= 0) return go; }
    if (const char *bad = kp_check_lists((size_t)count * c->d.dof, c->d.T, kp_offsets, kp_times)) return set_err(c, KPILQR_ERR_ARG, bad);
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "kpilqr_update_keypoints before kpilqr_set_keypoints / kpilqr_generate_keypoints");
    if (c->is_view) return set_err(c, KPILQR_ERR_STATE, kViewNeverAllocates);
    { const int rcp = check_complete(c, "kpilqr_update_keypoints"); if (rcp) return rcp; }
    const int rc = ensure_offsets_mirror(c);
    if (rc) return rc;
    return install_subset_lists(c, "kpilqr_update_keypoints", count, traj, kp_offsets, kp_times, 0);
}

// ---- key-point placement on the device ----------------------------------------------------------------
int kpilqr_upload_states(kpilqr_ctx *c, const double *X)
{
    KP_NOT_EMBEDDED(c, "kpilqr_upload_states");
    if (!c || !X) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    const size_t count = (size_t)c->d.batch * c->d.T * c->n;
    { const int rcg = reserve(c, c->X_states, count * sizeof(double), kExact, false); if (rcg < 0) return rcg; }
    KP_HIP(c, hipMemcpyAsync(c->X_states, X, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
    c->have_states = true;
    if (c->states_given_host) memset(c->states_given_host, 1, (size_t)c->d.batch);      // (no array yet: have_states says the same to whoever makes it)
    return KPILQR_OK;
}

// The placement arguments of kpilqr_generate_keypoints and kpilqr_generate_keypoints_partial -> the kernel's method number in *mth
// (0 set_interval, 1 adaptive_jerk, 2 velocity_change, 3 adaptive_accel), or KPILQR_ERR_ARG with the message
static int placement_args(kpilqr_ctx *c, const char *method, int min_N, int max_N, const double *thresholds, double dt, int *mth)
{
    if (strcmp(method, "set_interval") == 0) *mth = 0;
    else if (strcmp(method, "adaptive_jerk") == 0) *mth = 1;
    else if (strcmp(method, "velocity_change") == 0) *mth = 2;
    else if (strcmp(method, "adaptive_accel") == 0) *mth = 3;
    else return set_err(c, KPILQR_ERR_ARG, "kpilqr_generate_keypoints: method must be set_interval, adaptive_jerk, adaptive_accel or velocity_change "
                                           "(iterative_error interleaves host finite differences and stays on the host)");
    if (min_N < 1 || max_N < 1) return set_err(c, KPILQR_ERR_ARG, "min_N and max_N must be >= 1");
    if (c->d.dof > 64) return set_err(c, KPILQR_ERR_ARG, "on-device key-point placement supports dof <= 64");
    if (*mth != 0 && (!thresholds || (*mth == 1 && !(dt > 0.0)))) return set_err(c, KPILQR_ERR_ARG, "thresholds (and, for adaptive_jerk, a positive dt) are required");
    return KPILQR_OK;
}

int kpilqr_generate_keypoints(kpilqr_ctx *c, const char *method, int min_N, int max_N, const double *thresholds, double dt)
{
    KP_NOT_EMBEDDED(c, "kpilqr_generate_keypoints");
    if (!c || !method) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    int mth = -1;
    { const int rca = placement_args(c, method, min_N, max_N, thresholds, dt, &mth); if (rca) return rca; }
    if (mth != 0 && !c->have_states) return set_err(c, KPILQR_ERR_STATE, "kpilqr_generate_keypoints before kpilqr_upload_states");
    const size_t nlists = (size_t)c->d.batch * c->d.dof, T = c->d.T, nchunks = (T + 63) / 64;
    const struct { DevMem *buf; size_t bytes; } rows[] = {
        {&c->kp_thr, sizeof(double) * c->d.dof},
        {&c->kp_mask, sizeof(unsigned long long) * nlists * nchunks},
        {&c->kp_count, sizeof(int) * nlists},
        {&c->X_states, sizeof(double) * c->d.batch * T * c->n},      // set_interval never reads it
        {&c->kp_times, sizeof(int) * nlists * T},                    // worst case: every step a key-point
    };
    for (const auto &row : rows) { const int rcg = reserve(c, *row.buf, row.bytes, kExact, false); if (rcg < 0) return rcg; }
    if (thresholds) {
        KP_HIP(c, hipMemcpyAsync(c->kp_thr, thresholds, sizeof(double) * c->d.dof, hipMemcpyHostToDevice, c->stream));
        KP_HIP(c, hipStreamSynchronize(c->stream));       // the host array may be pageable
    }
    KP_HIP(c, launch_generate_keypoints(c, mth, min_N, max_N, dt, thresholds ? c->kp_thr : nullptr, c->X_states, c->kp_mask, c->kp_count));
    // The lists exist on the device only (kpilqr_get_keypoints brings them to the host), but their TOTAL is read back here --
    // one int: the column store and the entry tables are sized from it (not from the worst case batch * dof * T: 7.2 GB
    // against 1.4 GB at the headline shape), and the `entries` of a key-point ordered upload is checked against it.
    {
        int total = 0;
        KP_HIP(c, hipMemcpyAsync(&total, c->kp_offsets + nlists, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        KP_HIP(c, hipStreamSynchronize(c->stream));
        if (total < 0 || (size_t)total > nlists * T) return set_err(c, KPILQR_ERR_HIP, "kpilqr_generate_keypoints: implausible key-point count read back");
        // canonical: rows 0 and T-1 are always full and the lists are strictly increasing by construction; set_interval: one list
        // for all DoFs, the other methods place per DoF
        const int rci = lists_installed(c, total, true, mth == 0);
        if (rci) return rci;
    }
    if (c->kp_traj_first_host) { free(c->kp_traj_first_host); c->kp_traj_first_host = nullptr; }
    // (the lists exist on the device only: kpilqr_update_keypoints reads the offsets back when it first needs them)
    if (!remember_lists(c, nullptr)) return set_err(c, KPILQR_ERR_ALLOC, "host allocation failed");
    memset(c->kp_flags_host, kKpCanonical | (mth == 0 ? kKpUniform : 0), (size_t)c->d.batch);
    return KPILQR_OK;
}

int kpilqr_keypoint_error_test(kpilqr_ctx *c, int n_iv, const int *intervals, int min_N, double threshold, unsigned char *good)
{
    KP_NOT_EMBEDDED(c, "kpilqr_keypoint_error_test");
    if (!c || n_iv < 0 || (n_iv > 0 && (!intervals || !good))) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (n_iv == 0) return KPILQR_OK;
    const size_t iv_bytes = (size_t)n_iv * 4 * sizeof(int), off = (iv_bytes + 15) & ~(size_t)15;
    int rc = ensure_stage(c, off + (size_t)n_iv);
    if (rc) return rc;
    rc = ensure_records(c);                  // a fused context: records on demand, with the resident payload's columns
    if (rc) return rc;
    int *iv_dev = (int *)c->stage.p;
    unsigned char *good_dev = (unsigned char *)c->stage.p + off;
    KP_HIP(c, hipMemcpyAsync(iv_dev, intervals, iv_bytes, hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, launch_kp_error_test(c, n_iv, iv_dev, min_N, threshold, good_dev));
    KP_HIP(c, hipMemcpyAsync(good, good_dev, (size_t)n_iv, hipMemcpyDeviceToHost, c->stream));
    { const int rcs = sync_and_report(c); if (rcs) return rcs; }
    for (int k = 0; k < n_iv; k++) if (good[k] > 1) return set_err(c, KPILQR_ERR_ARG, "kpilqr_keypoint_error_test: interval out of range");
    return KPILQR_OK;
}

int kpilqr_get_keypoints(kpilqr_ctx *c, int *kp_offsets, int *kp_times, int times_capacity)
{
    KP_NOT_EMBEDDED(c, "kpilqr_get_keypoints");
    if (!c || !kp_offsets) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "no key-points set");
    const size_t nlists = (size_t)c->d.batch * c->d.dof;
    KP_HIP(c, hipMemcpyAsync(kp_offsets, c->kp_offsets, (nlists + 1) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    KP_HIP(c, hipStreamSynchronize(c->stream));
    const int total = kp_offsets[nlists];
    c->kp_total_host = total;
    (void)remember_traj_first(c, kp_offsets);          // (without it a streamed entry-ordered payload is refused, nothing else)
    if (kp_times) {
        if (total > times_capacity) return set_err(c, KPILQR_ERR_ARG, "kp_times capacity too small");
        KP_HIP(c, hipMemcpyAsync(kp_times, c->kp_times, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        KP_HIP(c, hipStreamSynchronize(c->stream));
    }
    return total;
}

static size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

static void fd_layout(int n, int njobs, int nnom, kpilqr_fd_layout *L)
{
    const size_t J = (size_t)njobs, N = (size_t)nnom;
    size_t o = 0;
    L->xplus = o; o = al16(o + J * n * sizeof(double));
    L->xminus = o; o = al16(o + J * n * sizeof(double));
    L->xnom = o; o = al16(o + N * n * sizeof(double));
    L->job_b = o; o = al16(o + J * sizeof(int));
    L->job_t = o; o = al16(o + J * sizeof(int));
    L->job_col = o; o = al16(o + J * sizeof(int));
    L->job_nom = o; o = al16(o + J * sizeof(int));
    L->job_mode = o; o = al16(o + J);
    L->bytes = o;
}

int kpilqr_fd_slab_layout(kpilqr_ctx *c, int njobs, int nnom, kpilqr_fd_layout *out)
{
    KP_NOT_EMBEDDED(c, "kpilqr_fd_slab_layout");
    if (!c || !out || njobs < 0 || nnom < 0) return KPILQR_ERR_ARG;
    fd_layout(c->n, njobs, nnom, out);
    return KPILQR_OK;
}

// device slab with the layout of (njobs, nnom); grows (with a stream sync) only when it has to
static int fd_bind(kpilqr_ctx *c, int njobs, int nnom, kpilqr_fd_layout *L)
{
    fd_layout(c->n, njobs, nnom, L);
    const int rc = reserve(c, c->fd_dev, L->bytes, kEighth, false);
    if (rc < 0) return rc;
    char *base = c->fd_dev;
    c->xplus = (double *)(base + L->xplus); c->xminus = (double *)(base + L->xminus); c->xnom = (double *)(base + L->xnom);
    c->job_b = (int *)(base + L->job_b); c->job_t = (int *)(base + L->job_t); c->job_col = (int *)(base + L->job_col);
    c->job_nom = (int *)(base + L->job_nom);
    c->job_mode = (unsigned char *)(base + L->job_mode);
    return KPILQR_OK;
}

int kpilqr_upload_fd(kpilqr_ctx *c, int njobs, const int *job_b, const int *job_t, const int *job_col,
                     const unsigned char *job_mode, const int *job_nom, const double *xplus,
                     const double *xminus, int nnom, const double *xnom, double eps)
{
    KP_NOT_EMBEDDED(c, "kpilqr_upload_fd");
    if (!c || njobs < 0 || nnom < 0) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (njobs > 0 && (!job_b || !job_t || !job_col || !job_mode || !xplus || !xminus))
        return set_err(c, KPILQR_ERR_ARG, "null FD job array");
    if (nnom > 0 && !xnom) return set_err(c, KPILQR_ERR_ARG, "nnom > 0 without xnom");
    if (!(eps > 0.0)) return set_err(c, KPILQR_ERR_ARG, "eps must be positive");
    const int n = c->n;
    kpilqr_fd_layout L;
    int rc = fd_bind(c, njobs, nnom, &L);
    if (rc) return rc;
    const size_t J = njobs;
    if (njobs) {
        KP_HIP(c, hipMemcpyAsync(c->job_b, job_b, J * sizeof(int), hipMemcpyHostToDevice, c->stream));
        KP_HIP(c, hipMemcpyAsync(c->job_t, job_t, J * sizeof(int), hipMemcpyHostToDevice, c->stream));
        KP_HIP(c, hipMemcpyAsync(c->job_col, job_col, J * sizeof(int), hipMemcpyHostToDevice, c->stream));
        KP_HIP(c, hipMemcpyAsync(c->job_mode, job_mode, J, hipMemcpyHostToDevice, c->stream));
        // no nominal rows given: every job_nom becomes -1, so a one-sided job (mode 1, 2) fails the device-side range check
        // whatever nnom is, is skipped and reported by the next synchronising call
        if (job_nom) KP_HIP(c, hipMemcpyAsync(c->job_nom, job_nom, J * sizeof(int), hipMemcpyHostToDevice, c->stream));
        else KP_HIP(c, hipMemsetAsync(c->job_nom, 0xff, J * sizeof(int), c->stream));
        KP_HIP(c, hipMemcpyAsync(c->xplus, xplus, J * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        KP_HIP(c, hipMemcpyAsync(c->xminus, xminus, J * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    if (nnom) KP_HIP(c, hipMemcpyAsync(c->xnom, xnom, (size_t)nnom * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    c->njobs = njobs; c->nnom = nnom; c->eps = eps;
    c->fd_payload = FdPayload::jobs; payload_changed(c);
    // pageable sources: the caller may free them on return, so wait for the copies; pinned ones are read in place
    if (!(is_pinned(job_b) && is_pinned(job_t) && is_pinned(job_col) && is_pinned(job_mode) && is_pinned(job_nom) &&
          is_pinned(xplus) && is_pinned(xminus) && is_pinned(xnom)))
        KP_HIP(c, hipStreamSynchronize(c->stream));
    return KPILQR_OK;
}

int kpilqr_upload_fd_slab(kpilqr_ctx *c, const void *slab, int njobs, int nnom, double eps)
{
    KP_NOT_EMBEDDED(c, "kpilqr_upload_fd_slab");
    if (!c || njobs < 0 || nnom < 0 || (njobs > 0 && !slab)) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (!(eps > 0.0)) return set_err(c, KPILQR_ERR_ARG, "eps must be positive");
    kpilqr_fd_layout L;
    int rc = fd_bind(c, njobs, nnom, &L);
    if (rc) return rc;
    if (njobs) KP_HIP(c, hipMemcpyAsync(c->fd_dev, slab, L.bytes, hipMemcpyHostToDevice, c->stream));   // the one DMA
    c->njobs = njobs; c->nnom = nnom; c->eps = eps;
    c->fd_payload = FdPayload::jobs; payload_changed(c);
    return wait_unless_pinned(c, slab);
}

// ---- key-point ordered FD payload ---------------------------------------------------------------------------------------
static void fdkp_layout(int n, int entries, kpilqr_fdkp_layout *L)
{
    L->entry_stride = (size_t)(6 * n + 2) * 8;
    L->xplus = 0; L->xminus = 8; L->elem_stride = 16; L->mode = (size_t)6 * n * 8;       // (x+, x-) pairs, element by element
    L->bytes = (size_t)entries * L->entry_stride;
}

int kpilqr_fd_kp_layout(kpilqr_ctx *c, int entries, kpilqr_fdkp_layout *out)
{
    if (!c || !out || entries < 0) return KPILQR_ERR_ARG;
    fdkp_layout(caller_n(c), entries, out);          // (an embedded context: the caller's records)
    return KPILQR_OK;
}

// device slab of the key-point ordered payload for `entries` entries; grows (after a stream sync) only when it has to
static int fdk_bind(kpilqr_ctx *c, int entries, kpilqr_fdkp_layout *L)
{
    fdkp_layout(c->n, entries, L);
    const int rc = reserve(c, c->fdk_dev, L->bytes, kEighth, false);
    return rc < 0 ? rc : KPILQR_OK;
}

int kpilqr_upload_fd_kp(kpilqr_ctx *c, const void *slab, int entries, double eps)
{
    if (!c || entries < 0 || (entries > 0 && !slab)) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (!(eps > 0.0)) return set_err(c, KPILQR_ERR_ARG, "eps must be positive");
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "kpilqr_upload_fd_kp before the key-points it is ordered by (kpilqr_set_keypoints / kpilqr_generate_keypoints)");
    // (the sweeps index the slab by the device CSR, not by `entries`: a smaller slab would be read past its end)
    if (entries != (c->embed.on ? c->emb_entries : c->kp_total_host))
        return set_err(c, KPILQR_ERR_ARG, "kpilqr_upload_fd_kp: `entries` is not the number of key-point entries (kp_offsets[batch*dof])");
    kpilqr_fdkp_layout L;
    int rc = KPILQR_OK;
    if (c->embed.on) {
        // the caller's records into the staging buffer with the one DMA, then one launch that writes every byte of the carrier's
        // records (embed.hip); the context is then what this call leaves on a context of the carrier's shape
        kpilqr_fdkp_layout own;
        fdkp_layout(caller_n(c), entries, &own);
        rc = ensure_emb_stage(c, own.bytes);
        if (rc) return rc;
        rc = fdk_bind(c, c->kp_total_host, &L);
        if (rc) return rc;
        if (entries) KP_HIP(c, hipMemcpyAsync(c->emb_stage, slab, own.bytes, hipMemcpyHostToDevice, c->stream));
        if (c->kp_total_host) KP_HIP(c, launch_embed_fd_kp(c, c->emb_stage));
        entries = c->kp_total_host;
    } else {
        rc = fdk_bind(c, entries, &L);
        if (rc) return rc;
        if (entries) KP_HIP(c, hipMemcpyAsync(c->fdk_dev, slab, L.bytes, hipMemcpyHostToDevice, c->stream));   // the one DMA
    }
    c->fdk_entries = entries; c->fdk_first = 0; c->eps = eps;
    c->fd_payload = FdPayload::kp_ordered; payload_changed(c);
    return wait_unless_pinned(c, slab);
}

// The differenced key-point columns as the payload (FdPayload::kp_columns): straight into the column store
int kpilqr_upload_kp_columns(kpilqr_ctx *c, const double *columns, int entries)
{
    if (!c || entries < 0 || (entries > 0 && !columns)) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "kpilqr_upload_kp_columns before the key-points it is ordered by (kpilqr_set_keypoints / kpilqr_generate_keypoints)");
    if (entries != (c->embed.on ? c->emb_entries : c->kp_total_host))
        return set_err(c, KPILQR_ERR_ARG, "kpilqr_upload_kp_columns: `entries` is not the number of key-point entries (kp_offsets[batch*dof])");
    int rc = KPILQR_OK;
    if (c->embed.on) {              // as kpilqr_upload_fd_kp: one DMA into the staging buffer, one launch straight into the column store
        const size_t own = (size_t)entries * 3 * caller_n(c) * 8;
        rc = ensure_emb_stage(c, own);
        if (rc) return rc;
        rc = ensure_kpc(c);
        if (rc) return rc;
        if (entries) KP_HIP(c, hipMemcpyAsync(c->emb_stage, columns, own, hipMemcpyHostToDevice, c->stream));
        if (c->kp_total_host) KP_HIP(c, launch_embed_kp_columns(c, (const double *)c->emb_stage.p));
        entries = c->kp_total_host;
    } else {
        rc = ensure_kpc(c);
        if (rc) return rc;
        if (entries) KP_HIP(c, hipMemcpyAsync(c->kpc, columns, (size_t)entries * 3 * c->n * 8, hipMemcpyHostToDevice, c->stream));
    }
    c->fd_payload = FdPayload::kp_columns; c->fdk_entries = entries; c->fdk_first = 0;      // (the entry range, as for the key-point ordered payload)
    payload_changed(c);
    c->pay.kpc_valid = true;
    return wait_unless_pinned(c, columns);
}

// ---- the pending ranges of kpilqr_update_keypoints filled in: one copy per run of adjacent trajectories, straight into place --------
// (entered through enter_subset(..., Subset::pending): `traj` is held against the pending set here, not against the batch)
static int check_partial(kpilqr_ctx *c, const char *who, FdPayload kind, int count, const int *traj, int entries)
{
    const std::string w(who);
    if (!payload_by_entry(c)) return set_err(c, KPILQR_ERR_STATE, w + ": no payload laid out by key-point entry is resident");
    if (c->fd_payload != kind) return set_err(c, KPILQR_ERR_STATE, w + ": the resident payload is of the other kind (key-point ordered records / key-point columns)");
    if (count != c->n_pending || (count > 0 && memcmp(traj, c->kp_pending_host, sizeof(int) * (size_t)count) != 0))
        return set_err(c, KPILQR_ERR_ARG, w + ": traj is not the set of trajectories pending since kpilqr_update_keypoints");
    if (entries != c->pending_entries) return set_err(c, KPILQR_ERR_ARG, w + ": `entries` is not the number of key-point entries of the listed trajectories");
    return KPILQR_OK;
}

static int upload_runs(kpilqr_ctx *c, int count, const int *traj, const char *src, char *dst, size_t rec_bytes)
{
    const int *first = c->kp_traj_first_host;
    return kp_for_each_run(count, traj, [&](int, int b0, int run) -> int {
        const size_t e0 = (size_t)first[b0], bytes = ((size_t)first[b0 + run] - e0) * rec_bytes;
        if (bytes) KP_HIP(c, hipMemcpyAsync(dst + e0 * rec_bytes, src, bytes, hipMemcpyHostToDevice, c->stream));
        src += bytes;
        return KPILQR_OK;
    });
}

int kpilqr_upload_fd_kp_partial(kpilqr_ctx *c, int count, const int *traj, const void *slab, int entries, double eps)
{
    KP_NOT_EMBEDDED(c, "kpilqr_upload_fd_kp_partial");
    if (entries < 0 || (entries > 0 && !slab)) return KPILQR_ERR_ARG;
    { const int go = enter_subset(c, "kpilqr_upload_fd_kp_partial", count, traj, Subset::pending); if (go <= 0) return go; }
    if (count == 0 && entries == 0 && !c->n_pending) return KPILQR_OK;
    int rc = check_partial(c, "kpilqr_upload_fd_kp_partial", FdPayload::kp_ordered, count, traj, entries);
    if (rc) return rc;
    if (memcmp(&eps, &c->eps, sizeof(double)) != 0)
        return set_err(c, KPILQR_ERR_ARG, "kpilqr_upload_fd_kp_partial: eps differs from the resident payload's (a context has one eps)");
    rc = upload_runs(c, count, traj, (const char *)slab, c->fdk_dev, c->fdk_stride());
    if (rc) return rc;
    payload_changed(c);                                  // complete again; whatever was derived from the old one is stale
    return wait_unless_pinned(c, slab);
}

int kpilqr_upload_kp_columns_partial(kpilqr_ctx *c, int count, const int *traj, const double *columns, int entries)
{
    KP_NOT_EMBEDDED(c, "kpilqr_upload_kp_columns_partial");
    if (entries < 0 || (entries > 0 && !columns)) return KPILQR_ERR_ARG;
    { const int go = enter_subset(c, "kpilqr_upload_kp_columns_partial", count, traj, Subset::pending); if (go <= 0) return go; }
    if (count == 0 && entries == 0 && !c->n_pending) return KPILQR_OK;
    int rc = check_partial(c, "kpilqr_upload_kp_columns_partial", FdPayload::kp_columns, count, traj, entries);
    if (rc) return rc;
    rc = upload_runs(c, count, traj, (const char *)columns, (char *)c->kpc.p, (size_t)3 * c->n * 8);
    if (rc) return rc;
    payload_changed(c);
    c->pay.kpc_valid = true;                                 // (the columns ARE the payload)
    return wait_unless_pinned(c, columns);
}

// ---- the key-point columns as FP32: half the bytes of the largest upload ---------------------------------------------------------------
// The encoded floats (include/kpilqr.h: A's unit entry removed before the cast) go with ONE copy into the staging buffer the context
// owns -- reserved on demand and kept at the largest size asked for, as the float buffer of the gains is -- and ONE launch
// (columns_f32.hip) widens them into the column store, adding the unit entry back.  The callers have checked everything.
static int reserve_columns_f32(kpilqr_ctx *c, int entries)
{
    const int rc = reserve(c, c->kpc32, (size_t)entries * 3 * c->n * sizeof(float), kExact, false);
    return rc < 0 ? rc : KPILQR_OK;
}

static int widen_columns_f32(kpilqr_ctx *c, const float *columns32, int entries, const int *upl_first)
{
    if (!entries) return KPILQR_OK;
    KP_HIP(c, hipMemcpyAsync(c->kpc32, columns32, (size_t)entries * 3 * c->n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, launch_kp_columns_f32(c, c->kpc32, upl_first));
    return KPILQR_OK;
}

int kpilqr_upload_kp_columns_f32(kpilqr_ctx *c, const float *columns32, int entries)
{
    KP_NOT_EMBEDDED(c, "kpilqr_upload_kp_columns_f32");
    if (!c || entries < 0 || (entries > 0 && !columns32)) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "kpilqr_upload_kp_columns_f32 before the key-points it is ordered by (kpilqr_set_keypoints / kpilqr_generate_keypoints)");
    if (entries != c->kp_total_host)
        return set_err(c, KPILQR_ERR_ARG, "kpilqr_upload_kp_columns_f32: `entries` is not the number of key-point entries (kp_offsets[batch*dof])");
    if (c->is_view) return set_err(c, KPILQR_ERR_STATE, "kpilqr_upload_kp_columns_f32: not through a view of a trajectory range");
    // both buffers before anything is enqueued or the context changes: the staging buffer first (it alone may fail for a context
    // whose column store is already there)
    int rc = reserve_columns_f32(c, entries);
    if (rc) return rc;
    rc = ensure_kpc(c);
    if (rc) return rc;
    rc = widen_columns_f32(c, columns32, entries, nullptr);
    if (rc) return rc;
    c->fd_payload = FdPayload::kp_columns; c->fdk_entries = entries; c->fdk_first = 0;      // (the state kpilqr_upload_kp_columns leaves)
    payload_changed(c);
    c->pay.kpc_valid = true;
    return wait_unless_pinned(c, columns32);
}

int kpilqr_upload_kp_columns_f32_partial(kpilqr_ctx *c, int count, const int *traj, const float *columns32, int entries)
{
    KP_NOT_EMBEDDED(c, "kpilqr_upload_kp_columns_f32_partial");
    if (entries < 0 || (entries > 0 && !columns32)) return KPILQR_ERR_ARG;
    { const int go = enter_subset(c, "kpilqr_upload_kp_columns_f32_partial", count, traj, Subset::pending); if (go <= 0) return go; }
    if (count == 0 && entries == 0 && !c->n_pending) return KPILQR_OK;
    int rc = check_partial(c, "kpilqr_upload_kp_columns_f32_partial", FdPayload::kp_columns, count, traj, entries);
    if (rc) return rc;
    if (c->is_view) return set_err(c, KPILQR_ERR_STATE, "kpilqr_upload_kp_columns_f32_partial: not through a view of a trajectory range");
    // The pending trajectories' entries inside `columns32` are the third row of the move table kpilqr_update_keypoints left on the
    // device (check_partial has held traj to exactly that call's list, and nothing else writes the table): the launch reads them
    // there, so a scattered list costs no copy per run
    rc = reserve_columns_f32(c, entries);
    if (rc) return rc;
    rc = widen_columns_f32(c, columns32, entries, (const int *)c->kp_move + 2 * ((size_t)c->d.batch + 1));
    if (rc) return rc;
    payload_changed(c);
    c->pay.kpc_valid = true;                                 // (the columns ARE the payload)
    return wait_unless_pinned(c, columns32);
}

int kpilqr_fd_difference(kpilqr_ctx *c)
{
    KP_NOT_EMBEDDED(c, "kpilqr_fd_difference");
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    { const int rcp = check_complete(c, "kpilqr_fd_difference"); if (rcp) return rcp; }
    if (c->fused) {
        // the sweeps read the key-point column store; the records, if something has asked for them, follow
        int rc = difference_to_kpc(c, !union_route(c));
        if (rc) return rc;
        return c->have_rec ? records_from_payload(c) : KPILQR_OK;
    }
    return records_from_payload(c);
}

int kpilqr_interpolate(kpilqr_ctx *c)
{
    KP_NOT_EMBEDDED(c, "kpilqr_interpolate");
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "kpilqr_interpolate before kpilqr_set_keypoints");
    { const int rcp = check_complete(c, "kpilqr_interpolate"); if (rcp) return rcp; }
    if (c->fused) { const int rc = ensure_records(c); if (rc) return rc; }
    KP_HIP(c, launch_interpolate(c));
    return KPILQR_OK;
}

// kpilqr_fd_difference + kpilqr_interpolate (Differentiator.cpp:166-222,441-457 + KeyPointGenerator.cpp:840-954)
int kpilqr_fd_interpolate(kpilqr_ctx *c)
{
    KP_NOT_EMBEDDED(c, "kpilqr_fd_interpolate");
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "kpilqr_fd_interpolate before kpilqr_set_keypoints");
    { const int rcp = check_complete(c, "kpilqr_fd_interpolate"); if (rcp) return rcp; }
    if (c->fused) {
        // the sweeps of a fused context read the column store: it is differenced as kpilqr_fd_difference does; the records appear on
        // demand (allocated and zeroed) and are filled in one pass where the payload allows
        int rc = difference_to_kpc(c, !union_route(c));
        if (rc) return rc;
        rc = ensure_record_storage(c);
        if (rc) return rc;
    }
    return linearise(c);
}

// Optimiser::FilterDynamicsMatrices (Optimiser.cpp:340-406) on the materialised A sequence
int kpilqr_filter_dynamics(kpilqr_ctx *c, const char *method, const double *coefs, int ncoef)
{
    KP_NOT_EMBEDDED(c, "kpilqr_filter_dynamics");
    if (!c || !method || !coefs) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    int mth = strcmp(method, "low_pass") == 0 ? 0 : strcmp(method, "FIR") == 0 ? 1 : -1;
    if (mth < 0) return set_err(c, KPILQR_ERR_ARG, "Filtering method not recognised (low_pass, FIR)");
    if (ncoef < 1 || ncoef > 16) return set_err(c, KPILQR_ERR_ARG, "1..16 filter coefficients");
    if (c->fused)
        return set_err(c, KPILQR_ERR_STATE, "the A filters act on the materialised sequence: create the context without KPILQR_FLAG_FUSED");
    int rc = ensure_stage(c, 16 * sizeof(double));
    if (rc) return rc;
    KP_HIP(c, hipMemcpyAsync(c->stage, coefs, sizeof(double) * ncoef, hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, hipStreamSynchronize(c->stream));
    KP_HIP(c, launch_filter_dynamics(c, mth, c->stage, ncoef));
    return KPILQR_OK;
}

// ---- STEP 1c ------------------------------------------------------------------------------------
int kpilqr_upload_residuals(kpilqr_ctx *c, const double *r, const double *r_x, const double *r_u,
                            const double *w_run, const double *w_term)
{
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    const size_t B = c->d.batch, T1 = c->d.T + 1, n = c->n, m = c->d.m, nr = c->d.nr;
    if (c->embed.on) {
        // r, w_run, w_term are shape-free; r_x and r_u cross in the caller's pitch into the staging buffer and one launch each places
        // their columns (embed.hip): the padding of the buffers was zeroed with them and is never written
        const size_t rows = B * T1 * nr, on = caller_n(c), om = caller_m(c);
        { const int rcs = ensure_emb_stage(c, rows * ((r_x ? on : 0) + (r_u ? om : 0)) * 8); if (rcs) return rcs; }
        double *const sx = (double *)c->emb_stage.p, *const su = sx + (r_x ? rows * on : 0);
        if (r) KP_HIP(c, hipMemcpyAsync(c->r, r, rows * 8, hipMemcpyHostToDevice, c->stream));
        if (r_x) {
            KP_HIP(c, hipMemcpyAsync(sx, r_x, rows * on * 8, hipMemcpyHostToDevice, c->stream));
            KP_HIP(c, launch_embed_rows(c, (long long)rows, (int)on, (int)n, c->embed.dof, c->embed.shift(c->d.dof), sx, c->r_x));
            c->rx_const_on = false; c->rx_buf_valid = c->rx_whole = true;
        }
        if (r_u) {
            KP_HIP(c, hipMemcpyAsync(su, r_u, rows * om * 8, hipMemcpyHostToDevice, c->stream));
            KP_HIP(c, launch_embed_rows(c, (long long)rows, (int)om, (int)m, (int)om, 0, su, c->r_u));
            c->ru_zero = false;
        }
        if (w_run) KP_HIP(c, hipMemcpyAsync(c->w_run, w_run, nr * 8, hipMemcpyHostToDevice, c->stream));
        if (w_term) KP_HIP(c, hipMemcpyAsync(c->w_term, w_term, nr * 8, hipMemcpyHostToDevice, c->stream));
        return KPILQR_OK;
    }
    if (r) KP_HIP(c, hipMemcpyAsync(c->r, r, B * T1 * nr * 8, hipMemcpyHostToDevice, c->stream));
    if (r_x) { KP_HIP(c, hipMemcpyAsync(c->r_x, r_x, B * T1 * nr * n * 8, hipMemcpyHostToDevice, c->stream)); c->rx_const_on = false; c->rx_buf_valid = c->rx_whole = true; }
    if (r_u) { KP_HIP(c, hipMemcpyAsync(c->r_u, r_u, B * T1 * nr * m * 8, hipMemcpyHostToDevice, c->stream)); c->ru_zero = false; }
    if (w_run) KP_HIP(c, hipMemcpyAsync(c->w_run, w_run, nr * 8, hipMemcpyHostToDevice, c->stream));
    if (w_term) KP_HIP(c, hipMemcpyAsync(c->w_term, w_term, nr * 8, hipMemcpyHostToDevice, c->stream));
    return KPILQR_OK;
}

// One r_x [nr][n] (and r_u [nr][m], or none) for every trajectory and step: a task whose residuals are affine in the state
// (reaching: r = [q - q*, qdot], Reaching.cpp:43-54).  Uploaded once; the fused one-wave sweeps then issue no r_x loads.
int kpilqr_upload_residual_jacobians_const(kpilqr_ctx *c, const double *r_x, const double *r_u)
{
    if (!c || !r_x) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    const size_t n = c->n, m = c->d.m, nr = c->d.nr, reps = (size_t)c->d.batch * (c->d.T + 1);
    // an embedded context: the one small matrix (and r_u's) padded on the host to the carrier's pitch; from here on the call is the
    // one a context of the carrier's shape gets, so rxc / ru0 are selected as there (the padded arrays are pageable: the call waits)
    std::vector<double> px, pu;
    if (c->embed.on) {
        const size_t on = caller_n(c), om = caller_m(c), dof = c->embed.dof, shift = c->embed.shift(c->d.dof);
        px.assign(nr * n, 0.0);
        for (size_t i = 0; i < nr; i++)
            for (size_t j = 0; j < on; j++) px[i * n + (j < dof ? j : j + shift)] = r_x[i * on + j];
        r_x = px.data();
        if (r_u) {
            pu.assign(nr * m, 0.0);
            for (size_t i = 0; i < nr; i++)
                for (size_t j = 0; j < om; j++) pu[i * m + j] = r_u[i * om + j];
            r_u = pu.data();
        }
    }
    { const int rcg = reserve(c, c->rx_const, nr * n * 8, kExact, false); if (rcg < 0) return rcg; }
    KP_HIP(c, hipMemcpyAsync(c->rx_const, r_x, nr * n * 8, hipMemcpyHostToDevice, c->stream));
    c->rx_const_on = true; c->rx_buf_valid = false;
    if (r_u) {                                   // dense control residuals: streamed from the (broadcast) buffer like r_x then
        const int rcs = ensure_stage(c, nr * m * 8);
        if (rcs) return rcs;
        KP_HIP(c, hipMemcpyAsync(c->stage, r_u, nr * m * 8, hipMemcpyHostToDevice, c->stream));
        KP_HIP(c, launch_broadcast(c->stream, c->stage, (int)(nr * m), c->r_u, reps));
        c->ru_zero = false;
    } else if (!c->ru_zero) {
        KP_HIP(c, hipMemsetAsync(c->r_u, 0, reps * nr * m * 8, c->stream));
        c->ru_zero = true;
    }
    if (!(is_pinned(r_x) && is_pinned(r_u))) KP_HIP(c, hipStreamSynchronize(c->stream));
    return KPILQR_OK;
}

int kpilqr_cost_derivs(kpilqr_ctx *c)
{
    KP_NOT_EMBEDDED(c, "kpilqr_cost_derivs");
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    { const int rcx = ensure_rx_buffer(c); if (rcx) return rcx; }
    if (c->fused) { const int rc = ensure_records(c); if (rc) return rc; }
    KP_HIP(c, launch_cost_derivs(c));
    return KPILQR_OK;
}

int kpilqr_trajectory_cost(kpilqr_ctx *c, double *cost)
{
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    KP_HIP(c, launch_trajectory_cost(c));
    if (cost) KP_HIP(c, hipMemcpyAsync(cost, c->traj_cost, (size_t)c->d.batch * 8, hipMemcpyDeviceToHost, c->stream));
    return KPILQR_OK;
}

// ---- STEP 2 -------------------------------------------------------------------------------------
static int check_fused(kpilqr_ctx *c)
{
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "fused sweeps need kpilqr_set_keypoints first");
    if (!c->kp_canonical)
        return set_err(c, KPILQR_ERR_STATE, "fused sweeps need canonical key-points (per DoF: strictly increasing, first 0, last T-1)");
    return KPILQR_OK;
}

// ---- the lambda retry schedule (kpilqr_set_lambda_retry) --------------------------------------------------------------------
// How many attempts a backward pass launches: the longest run of lambda values the schedule allows from the lambdas the caller passed
// (for positive lambdas: from the smallest), the host loop's multiply and comparison, capped by max_attempts.  Without the caller's
// lambdas (the resident ones are used) max_attempts.  Later attempts than a trajectory needs leave at the gate.
static int retry_attempts_for(const kpilqr_ctx *c, const double *lambda, size_t count)
{
    if (!c->retry_on) return 1;
    const kpilqr_lambda_retry &s = c->retry;
    if (!lambda) return s.max_attempts;
    int most = 1;
    for (size_t b = 0; b < count && most < s.max_attempts; b++) {
        int a = 1;
        for (double l = lambda[b]; a < s.max_attempts; a++) {
            l = l * s.factor;
            if (l > s.max_lambda) break;
        }
        if (a > most) most = a;
    }
    return most;
}

// The sweep launch of one backward pass -- `launch`, a launcher's whole launch sequence on lc (the context, a chunk view, or the union
// view made from c) -- and under a schedule its repetitions: k_lambda_retry between two attempts advances lambda where a PD check
// failed and writes the gate the next attempt's kernels look at first.  The first attempt has no gate: it is the launch of a context
// without a schedule.  What runs before the sweeps (column store, slopes, broadcast Jacobians) has run once, in run_backward.
extern "C++" template <class Launch>
static int sweep_attempts(kpilqr_ctx *c, kpilqr_ctx *lc, Launch launch)
{
    // A listed launch (lc: make_list_view) runs through the GATED instantiations from its first attempt on -- they are the ones that read
    // the list beside the gate -- with the gate armed for the listed trajectories alone; the schedule's two kernels walk the list, not the batch.
    const bool listed = lc->sweep_list != nullptr;
    const int *const first_gate = listed ? (const int *)c->gate : nullptr;
    kpilqr_ctx *const rc = listed ? lc : c;
    lc->bwd_gate = first_gate;
    if (!c->retry_on) {
        if (listed) KP_HIP(c, launch_gate_arm(lc));
        KP_HIP(c, launch());
        return KPILQR_OK;
    }
    KP_HIP(c, launch_lambda_retry_begin(rc));
    KP_HIP(c, launch());
    for (int a = 1; a < c->retry_attempts; a++) {
        KP_HIP(c, launch_lambda_retry(rc));
        lc->bwd_gate = c->gate;
        const hipError_t e = launch();
        lc->bwd_gate = first_gate;
        KP_HIP(c, e);
    }
    c->retry_ran = true;
    return KPILQR_OK;
}

// the sweep of a context that is not fused, on lc (the context, or a list view of it): one launcher per family
static hipError_t launch_backward_family(Ctx *lc, int pd_stride)
{
    switch (lc->bwd_family) {
    case Family::t1: return launch_backward_mfma(lc, pd_stride);
    case Family::tiled: return launch_backward_tiled(lc, pd_stride);
    case Family::wide: return launch_backward_wide(lc, pd_stride);
    default: return launch_backward_generic(lc, pd_stride);
    }
}

static int run_backward(kpilqr_ctx *c, int pd_stride)
{
    c->last_width[0] = -1;
    if (c->fused) {
        int rc = check_fused(c);
        if (rc) return rc;
        if (union_route(c)) {
            rc = prepare_union(c);
            if (rc) return rc;
            kpilqr_ctx v;
            make_union_view(c, &v);
            FusedLaunch plan = plan_backward_fused(&v, false);
            plan.uni_on_union = true;
            c->last_bwd = plan;
            if (!plan.rxc) { rc = ensure_rx_buffer(c); if (rc) return rc; }
            return sweep_attempts(c, &v, [&] { return launch_backward_fused(&v, plan, pd_stride); });
        }
        rc = ensure_kpc(c);
        if (rc) return rc;
        rc = ensure_kps(c);
        if (rc) return rc;
        // Key-point ordered payload: the sweep (one wave per trajectory, or the helper wave of the pair) differences the payload
        // itself and leaves kpc behind for the forward sweep -- no differencing kernel.  (It may stop at a failed PD check, so it
        // never marks kpc valid: another backward pass on the same payload differences again.)  Otherwise the payload is
        // differenced into kpc first, once, and the sweeps read kpc.
        const FusedLaunch plan = c->last_bwd = plan_backward_fused(c, !c->pay.kpc_valid && c->fd_payload == FdPayload::kp_ordered && c->tune.fused_raw != 0);
        if (!plan.rxc) { rc = ensure_rx_buffer(c); if (rc) return rc; }       // (the sweep streams r_x: a constant one needs its broadcast copy)
        if (plan.raw) {
            // (a retried raw sweep differences its trajectory's payload again, as it does after a retry by the host)
            rc = sweep_attempts(c, c, [&] { return launch_backward_fused(c, plan, pd_stride); });
            if (rc) return rc;
            c->pay.kpc_touched = true;
            // (KPILQR_FUSED_UNI=0, diagnostic: the GENERAL raw sweep has differenced every set inside the sweep -- dividing at its
            // crossings -- and left the columns; the forward sweep's general form walks the slope store, made from them here)
            if (c->kps && !plan.slopes) KP_HIP(c, launch_kp_slopes(c, false));
            return KPILQR_OK;
        }
        if (!c->pay.kpc_valid) { rc = difference_to_kpc(c); if (rc) return rc; }
        if (c->pay.kpc_valid) { rc = slopes_for_kpc(c); if (rc) return rc; }
        return sweep_attempts(c, c, [&] { return launch_backward_fused(c, plan, pd_stride); });
    }
    c->last_bwd = FusedLaunch{};       // (no plan: not a fused launch, and the tiled a6 sweep streams r_x)
    if (c->tiled_a6) { const int rc = ensure_rx_buffer(c); if (rc) return rc; }
    return sweep_attempts(c, c, [&] { return launch_backward_family(c, pd_stride); });
}

int kpilqr_backward(kpilqr_ctx *c, const double *lambda, int pd_check_stride, int *status, double *delta_J)
{
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (pd_check_stride < 1) return set_err(c, KPILQR_ERR_ARG, "pd_check_stride must be >= 1");
    { const int rcp = check_complete(c, "kpilqr_backward"); if (rcp) return rcp; }
    { const int rcl = check_embedded_lambda(c, "kpilqr_backward", lambda); if (rcl) return rcl; }
    if (lambda) KP_HIP(c, hipMemcpyAsync(c->lambda, lambda, (size_t)c->d.batch * 8, hipMemcpyHostToDevice, c->stream));
    c->retry_attempts = retry_attempts_for(c, lambda, c->d.batch);
    int rc = run_backward(c, pd_check_stride);
    if (rc) return rc;
    if (status) KP_HIP(c, hipMemcpyAsync(status, c->status, (size_t)c->d.batch * 4, hipMemcpyDeviceToHost, c->stream));
    if (delta_J) KP_HIP(c, hipMemcpyAsync(delta_J, c->delta_J, (size_t)c->d.batch * 8, hipMemcpyDeviceToHost, c->stream));
    return KPILQR_OK;
}

// Diagnostic (bench's lambda sweep): the backward pass of a fused context in its instrumented form.  hist [batch][6] = number
// of steps whose (Quu + lambda I)^-1 came from: the third-order Newton-Schulz refresh alone, that plus 1 / 2 / 3 second-order
// steps, the LDL' factorisation (first step, checked steps, re-seeds), the pivoted slow path.  Gains, delta_J and status
// are written as by kpilqr_backward.  Uses the lambda already resident.  Synchronous.  One sweep whatever kpilqr_set_lambda_retry says:
// the instrumented kernel has no gate, and the histogram is that of ONE sweep.
int kpilqr_backward_stats(kpilqr_ctx *c, int pd_check_stride, int *hist)
{
    KP_NOT_EMBEDDED(c, "kpilqr_backward_stats");
    if (!c || !hist) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (!c->fused) return set_err(c, KPILQR_ERR_STATE, "kpilqr_backward_stats: fused contexts only");
    if (pd_check_stride < 1) return set_err(c, KPILQR_ERR_ARG, "pd_check_stride must be >= 1");
    { const int rcp = check_complete(c, "kpilqr_backward_stats"); if (rcp) return rcp; }
    int rc = check_fused(c);
    if (rc) return rc;
    rc = ensure_kpc(c);
    if (rc) return rc;
    if (!c->pay.kpc_valid) { rc = difference_to_kpc(c); if (rc) return rc; }
    // (the instrumented sweep is the GENERAL form whatever the lists are: it walks the slope store, made here unconditionally)
    rc = ensure_kps(c, true);
    if (rc) return rc;
    rc = slopes_for_kpc(c, true);
    if (rc) return rc;
    rc = ensure_rx_buffer(c);
    if (rc) return rc;
    const size_t bytes = (size_t)c->d.batch * 6 * sizeof(int);
    rc = ensure_stage(c, bytes);
    if (rc) return rc;
    KP_HIP(c, launch_backward_fused_stats(c, pd_check_stride, (int *)c->stage.p));
    KP_HIP(c, hipMemcpyAsync(hist, c->stage, bytes, hipMemcpyDeviceToHost, c->stream));
    return sync_and_report(c);
}

// The lambda retry schedule (include/kpilqr.h, "Lambda retry").  Everything is checked before the context changes; nothing is enqueued.
int kpilqr_set_lambda_retry(kpilqr_ctx *c, const kpilqr_lambda_retry *sched)
{
    if (!c) return KPILQR_ERR_ARG;
    if (c->is_view) return set_err(c, KPILQR_ERR_ARG, "kpilqr_set_lambda_retry: not through a view of a trajectory range");
    if (sched) {
        if (sched->struct_size != sizeof(kpilqr_lambda_retry))
            return set_err(c, KPILQR_ERR_ARG, "kpilqr_set_lambda_retry: struct_size is not sizeof(kpilqr_lambda_retry) of this library");
        // (written so that a NaN fails each test)
        if (!(sched->factor > 1.0) || !(sched->factor <= 1.7976931348623157e308))
            return set_err(c, KPILQR_ERR_ARG, "kpilqr_set_lambda_retry: factor must be finite and > 1");
        if (!(sched->max_lambda > 0.0) || !(sched->max_lambda <= 1.7976931348623157e308))
            return set_err(c, KPILQR_ERR_ARG, "kpilqr_set_lambda_retry: max_lambda must be finite and > 0");
        if (sched->max_attempts < 1 || sched->max_attempts > 64)
            return set_err(c, KPILQR_ERR_ARG, "kpilqr_set_lambda_retry: max_attempts must be in 1 .. 64");
    }
    // (a streamed iteration in flight has enqueued its attempts already: the new schedule holds from the next call on)
    c->retry_on = sched != nullptr;
    c->retry = sched ? *sched : kpilqr_lambda_retry{};
    c->retry_ran = false;
    c->retry_attempts = 1;
    return KPILQR_OK;
}

int kpilqr_download_lambda_retry(kpilqr_ctx *c, double *lambda_used, int *attempts)
{
    if (!c) return KPILQR_ERR_ARG;
    if (c->is_view) return set_err(c, KPILQR_ERR_ARG, "kpilqr_download_lambda_retry: not through a view of a trajectory range");
    if (!c->retry_on) return set_err(c, KPILQR_ERR_STATE, "kpilqr_download_lambda_retry: no schedule is set (kpilqr_set_lambda_retry)");
    if (!c->retry_ran) return set_err(c, KPILQR_ERR_STATE, "kpilqr_download_lambda_retry: no backward sweep has run under the schedule yet");
    KP_ENTER(c);              // (behind the chunks of a streamed iteration in flight)
    if (lambda_used) KP_HIP(c, hipMemcpyAsync(lambda_used, c->lambda, (size_t)c->d.batch * 8, hipMemcpyDeviceToHost, c->stream));
    if (attempts) KP_HIP(c, hipMemcpyAsync(attempts, c->attempts, (size_t)c->d.batch * 4, hipMemcpyDeviceToHost, c->stream));
    return KPILQR_OK;
}

// The gains of an embedded context: ONE launch per array gathers the real block of the carrier's K [b][T][n'][m'] (k: [b][T][m'])
// into the compact staging buffer in the caller's shape -- K as FP32 by the cast of k_gains_f32 when asked -- and ONE copy per array
// takes it to the host: no strided copies of 8 m-byte rows.
static int download_embedded_gains(kpilqr_ctx *c, void *K, bool K_f32, double *k)
{
    const size_t B = c->d.batch, T = c->d.T, on = caller_n(c), om = caller_m(c);
    const size_t bytesK = K ? B * T * on * om * (K_f32 ? 4 : 8) : 0, offk = (bytesK + 15) & ~(size_t)15, bytesk = k ? B * T * om * 8 : 0;
    { const int rcs = ensure_emb_stage(c, offk + bytesk); if (rcs) return rcs; }
    if (K) {
        KP_HIP(c, launch_extract_gains(c, (int)B, (long long)T, (int)on, (int)om, c->n, c->d.m, c->embed.dof, c->embed.shift(c->d.dof), c->K, c->emb_stage.p, K_f32));
        KP_HIP(c, hipMemcpyAsync(K, c->emb_stage.p, bytesK, hipMemcpyDeviceToHost, c->stream));
    }
    if (k) {
        KP_HIP(c, launch_extract_gains(c, (int)B, (long long)T, 1, (int)om, 1, c->d.m, 1, 0, c->k, (char *)c->emb_stage.p + offk, false));
        KP_HIP(c, hipMemcpyAsync(k, (char *)c->emb_stage.p + offk, bytesk, hipMemcpyDeviceToHost, c->stream));
    }
    return KPILQR_OK;
}

int kpilqr_download_gains(kpilqr_ctx *c, double *K, double *k)
{
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (c->embed.on) return download_embedded_gains(c, K, false, k);
    const size_t B = c->d.batch, T = c->d.T, n = c->n, m = c->d.m;
    if (K) KP_HIP(c, hipMemcpyAsync(K, c->K, B * T * n * m * 8, hipMemcpyDeviceToHost, c->stream));
    if (k) KP_HIP(c, hipMemcpyAsync(k, c->k, B * T * m * 8, hipMemcpyDeviceToHost, c->stream));
    return KPILQR_OK;
}

// the gains of the listed trajectories, compact: one copy per array and run of adjacent trajectories
int kpilqr_download_gains_partial(kpilqr_ctx *c, int count, const int *traj, double *K, double *k)
{
    KP_NOT_EMBEDDED(c, "kpilqr_download_gains_partial");
    { const int go = enter_subset(c, "kpilqr_download_gains_partial", count, traj, Subset::listed_or_view); if (go <= 0) return go; }
    const size_t perK = (size_t)c->d.T * c->n * c->d.m, perk = (size_t)c->d.T * c->d.m;
    return kp_for_each_run(count, traj, [&](int i, int b0, int run) -> int {
        if (K) KP_HIP(c, hipMemcpyAsync(K + (size_t)i * perK, c->K + (size_t)b0 * perK, (size_t)run * perK * 8, hipMemcpyDeviceToHost, c->stream));
        if (k) KP_HIP(c, hipMemcpyAsync(k + (size_t)i * perk, c->k + (size_t)b0 * perk, (size_t)run * perk * 8, hipMemcpyDeviceToHost, c->stream));
        return KPILQR_OK;
    });
}

// iLQR_SVR::LeastImportantDofs, summing branch (iLQR_SVR.cpp:952-968), over the gains of the last backward pass
int kpilqr_dof_importance(kpilqr_ctx *c, int sampling_k_interval, double *sums)
{
    KP_NOT_EMBEDDED(c, "kpilqr_dof_importance");
    if (!c || !sums) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (sampling_k_interval < 1) return set_err(c, KPILQR_ERR_ARG, "sampling_k_interval must be >= 1");
    const size_t bytes = (size_t)c->d.batch * c->d.dof * sizeof(double);
    int rc = ensure_stage(c, bytes);
    if (rc) return rc;
    KP_HIP(c, launch_dof_importance(c, sampling_k_interval, c->stage));
    KP_HIP(c, hipMemcpyAsync(sums, c->stage, bytes, hipMemcpyDeviceToHost, c->stream));
    return KPILQR_OK;
}

// iLQR_SVR::LeastImportantDofs, singular-vector branch (iLQR_SVR.cpp:902-950), over the gains of the last backward pass
int kpilqr_dof_importance_svd(kpilqr_ctx *c, int sampling_k_interval, double *sums)
{
    KP_NOT_EMBEDDED(c, "kpilqr_dof_importance_svd");
    if (!c || !sums) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (sampling_k_interval < 1) return set_err(c, KPILQR_ERR_ARG, "sampling_k_interval must be >= 1");
    if (!svr_supported(c->n, c->d.m)) return set_err(c, KPILQR_ERR_ARG, "kpilqr_dof_importance_svd: n * m too large for the LDS of one wave");
    int rc = ensure_stage(c, svr_stage_bytes(c->d.batch, c->d.dof, c->d.m, c->d.T, sampling_k_interval));
    if (rc) return rc;
    KP_HIP(c, launch_dof_importance_svd(c, sampling_k_interval, c->stage));
    KP_HIP(c, hipMemcpyAsync(sums, c->stage, (size_t)c->d.batch * c->d.dof * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return KPILQR_OK;
}

// ---- STEP 3 -------------------------------------------------------------------------------------
int kpilqr_upload_nominal(kpilqr_ctx *c, const double *u_nom, const double *ctrl_lim)
{
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    const size_t B = c->d.batch, T = c->d.T, m = c->d.m;
    if (c->embed.on) {
        // u_nom to the carrier's pitch through the staging buffer and k_embed_rows (the padded controls stay +0); the limits of the
        // padded controls are (-1, 1), set on the host (2 m' doubles from a temporary: the call waits for that copy)
        const size_t om = caller_m(c);
        if (u_nom) {
            { const int rcs = ensure_emb_stage(c, B * T * om * 8); if (rcs) return rcs; }
            KP_HIP(c, hipMemcpyAsync(c->emb_stage, u_nom, B * T * om * 8, hipMemcpyHostToDevice, c->stream));
            KP_HIP(c, launch_embed_rows(c, (long long)(B * T), (int)om, (int)m, (int)om, 0, (const double *)c->emb_stage.p, c->u_nom));
        }
        if (ctrl_lim) {
            std::vector<double> lim(2 * m);
            for (size_t j = 0; j < m; j++) { lim[2 * j] = j < om ? ctrl_lim[2 * j] : -1.0; lim[2 * j + 1] = j < om ? ctrl_lim[2 * j + 1] : 1.0; }
            KP_HIP(c, hipMemcpyAsync(c->ctrl_lim, lim.data(), 2 * m * 8, hipMemcpyHostToDevice, c->stream));
            KP_HIP(c, hipStreamSynchronize(c->stream));
        }
        return KPILQR_OK;
    }
    if (u_nom) KP_HIP(c, hipMemcpyAsync(c->u_nom, u_nom, B * T * m * 8, hipMemcpyHostToDevice, c->stream));
    if (ctrl_lim) KP_HIP(c, hipMemcpyAsync(c->ctrl_lim, ctrl_lim, 2 * m * 8, hipMemcpyHostToDevice, c->stream));
    return KPILQR_OK;
}

// ---- partial re-linearisation, the rest: residuals, nominal controls and step records of SOME trajectories ------------------------
// `per` doubles per trajectory, compact on the host in traj order: one copy per run of adjacent trajectories, straight to their place
static int upload_rows(kpilqr_ctx *c, int count, const int *traj, const double *src, double *dst, size_t per)
{
    return kp_for_each_run(count, traj, [&](int i, int b0, int run) -> int {
        KP_HIP(c, hipMemcpyAsync(dst + (size_t)b0 * per, src + (size_t)i * per, (size_t)run * per * 8, hipMemcpyHostToDevice, c->stream));
        return KPILQR_OK;
    });
}

int kpilqr_upload_residuals_partial(kpilqr_ctx *c, int count, const int *traj, const double *r, const double *r_x, const double *r_u)
{
    KP_NOT_EMBEDDED(c, "kpilqr_upload_residuals_partial");
    int rc = enter_subset(c, "kpilqr_upload_residuals_partial", count, traj);
    if (rc <= 0) return rc;
    // rows of a subset need every other row of the buffer to mean something, and must not flip the form the sweeps run in
    if (r_x && c->rx_const_on)
        return set_err(c, KPILQR_ERR_STATE, "kpilqr_upload_residuals_partial: the context holds constant residual Jacobians; a whole r_x through kpilqr_upload_residuals ends that mode first");
    if (r_x && !(c->rx_buf_valid && c->rx_whole))
        return set_err(c, KPILQR_ERR_STATE, "kpilqr_upload_residuals_partial: r_x of a subset before a whole r_x: kpilqr_upload_residuals first");
    if (r_u && c->ru_zero)
        return set_err(c, KPILQR_ERR_STATE, "kpilqr_upload_residuals_partial: r_u of a subset on a context that runs without control residuals: a whole r_u through kpilqr_upload_residuals first");
    const size_t T1 = c->d.T + 1, n = c->n, m = c->d.m, nr = c->d.nr;
    if (r) { rc = upload_rows(c, count, traj, r, c->r, T1 * nr); if (rc) return rc; }
    if (r_x) { rc = upload_rows(c, count, traj, r_x, c->r_x, T1 * nr * n); if (rc) return rc; }
    if (r_u) { rc = upload_rows(c, count, traj, r_u, c->r_u, T1 * nr * m); if (rc) return rc; }
    return KPILQR_OK;
}

// ---- the per-step residual Jacobians as FP32: half the bytes of the largest upload of a task whose residuals are not affine ---------
// The floats (include/kpilqr.h: a plain cast, nothing is encoded) go with ONE copy per array into the staging buffer the context owns
// -- [r_x32 | r_u32], reserved on demand and kept at the largest size asked for, as the staging buffer of the FP32 columns is -- and
// ONE launch per array (residuals_f32.hip) widens them into r_x / r_u, at the listed trajectories' rows for the partial call: the
// kernel places the rows, so a scattered list costs no copy per run.  The callers have checked everything; `rows` trajectories are
// compact in the caller's arrays, list == nullptr: they are trajectories 0 .. rows-1.
static int widen_residual_jacobians_f32(kpilqr_ctx *c, int rows, const int *list, const float *r_x32, const float *r_u32)
{
    const size_t T1 = c->d.T + 1, nr = c->d.nr, perx = T1 * nr * c->n, peru = T1 * nr * c->d.m;
    const size_t nx = r_x32 ? (size_t)rows * perx : 0, nu = r_u32 ? (size_t)rows * peru : 0;
    // the staging buffer before anything is enqueued or the context changes (KPILQR_ERR_ALLOC leaves the context as it was)
    { const int rcs = reserve(c, c->rj32, (nx + nu) * sizeof(float), kExact, false); if (rcs < 0) return rcs; }
    if (!(nx + nu)) return KPILQR_OK;
    const int *list_dev = nullptr;
    if (list) {
        KP_HIP(c, hipMemcpyAsync(c->traj_list, list, (size_t)rows * sizeof(int), hipMemcpyHostToDevice, c->stream));
        list_dev = c->traj_list;
    }
    float *const sx = c->rj32, *const su = sx + nx;           // (nx is even: r_u32's floats start on a pair)
    if (nx) {
        KP_HIP(c, hipMemcpyAsync(sx, r_x32, nx * sizeof(float), hipMemcpyHostToDevice, c->stream));
        KP_HIP(c, launch_widen_rows(c, list_dev, rows, (long long)perx, sx, c->r_x));
    }
    if (nu) {
        KP_HIP(c, hipMemcpyAsync(su, r_u32, nu * sizeof(float), hipMemcpyHostToDevice, c->stream));
        KP_HIP(c, launch_widen_rows(c, list_dev, rows, (long long)peru, su, c->r_u));
    }
    return KPILQR_OK;
}

int kpilqr_upload_residual_jacobians_f32(kpilqr_ctx *c, const float *r_x32, const float *r_u32)
{
    KP_NOT_EMBEDDED(c, "kpilqr_upload_residual_jacobians_f32");
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (c->is_view) return set_err(c, KPILQR_ERR_STATE, "kpilqr_upload_residual_jacobians_f32: not through a view of a trajectory range");
    if (!r_x32 && !r_u32) return KPILQR_OK;
    const int rc = widen_residual_jacobians_f32(c, c->d.batch, nullptr, r_x32, r_u32);
    if (rc) return rc;
    // (the state kpilqr_upload_residuals leaves)
    if (r_x32) { c->rx_const_on = false; c->rx_buf_valid = c->rx_whole = true; }
    if (r_u32) c->ru_zero = false;
    if (!(is_pinned(r_x32) && is_pinned(r_u32))) KP_HIP(c, hipStreamSynchronize(c->stream));
    return KPILQR_OK;
}

int kpilqr_upload_residual_jacobians_f32_partial(kpilqr_ctx *c, int count, const int *traj, const float *r_x32, const float *r_u32)
{
    KP_NOT_EMBEDDED(c, "kpilqr_upload_residual_jacobians_f32_partial");
    int rc = enter_subset(c, "kpilqr_upload_residual_jacobians_f32_partial", count, traj);        // (refuses a view, as every listed call)
    if (rc <= 0) return rc;
    // (the refusals of kpilqr_upload_residuals_partial, in its words)
    if (r_x32 && c->rx_const_on)
        return set_err(c, KPILQR_ERR_STATE, "kpilqr_upload_residual_jacobians_f32_partial: the context holds constant residual Jacobians; a whole r_x through kpilqr_upload_residuals ends that mode first");
    if (r_x32 && !(c->rx_buf_valid && c->rx_whole))
        return set_err(c, KPILQR_ERR_STATE, "kpilqr_upload_residual_jacobians_f32_partial: r_x of a subset before a whole r_x: kpilqr_upload_residuals first");
    if (r_u32 && c->ru_zero)
        return set_err(c, KPILQR_ERR_STATE, "kpilqr_upload_residual_jacobians_f32_partial: r_u of a subset on a context that runs without control residuals: a whole r_u through kpilqr_upload_residuals first");
    if (!r_x32 && !r_u32) return KPILQR_OK;
    rc = widen_residual_jacobians_f32(c, count, traj, r_x32, r_u32);
    if (rc) return rc;
    if (!(is_pinned(r_x32) && is_pinned(r_u32))) KP_HIP(c, hipStreamSynchronize(c->stream));
    return KPILQR_OK;
}

int kpilqr_upload_nominal_partial(kpilqr_ctx *c, int count, const int *traj, const double *u_nom)
{
    KP_NOT_EMBEDDED(c, "kpilqr_upload_nominal_partial");
    const int go = enter_subset(c, "kpilqr_upload_nominal_partial", count, traj);
    if (go <= 0) return go;
    return u_nom ? upload_rows(c, count, traj, u_nom, c->u_nom, (size_t)c->d.T * c->d.m) : KPILQR_OK;
}

// The key-point columns of the listed trajectories alone written into the records (the middle pass of the three-pass sequence on
// a payload laid out by entry): a trajectory's entries are one range of the column store, so this is k_kpc_to_records once per run
// of adjacent trajectories.  Only KPILQR_FD_INTERP=0 comes here -- a diagnostic switch; the product path is the one pass.
static int kpc_to_records_of(kpilqr_ctx *c, int count, const int *traj)
{
    if (!c->kp_traj_first_host) {             // (lists placed on the device: their offsets are read back, once)
        const int rc = ensure_offsets_mirror(c);
        if (rc) return rc;
        if (!remember_traj_first(c, c->kp_offsets_host)) return set_err(c, KPILQR_ERR_ALLOC, "host allocation failed");
    }
    const int *first = c->kp_traj_first_host;
    return kp_for_each_run(count, traj, [&](int, int b0, int run) -> int {
        KP_HIP(c, launch_kpc_to_records(c, first[b0], first[b0 + run] - first[b0]));
        return KPILQR_OK;
    });
}

// kpilqr_fd_interpolate for the listed trajectories: [A|B] of their records from the resident payload, nobody else's records written
int kpilqr_fd_interpolate_partial(kpilqr_ctx *c, int count, const int *traj)
{
    KP_NOT_EMBEDDED(c, "kpilqr_fd_interpolate_partial");
    int rc = enter_subset(c, "kpilqr_fd_interpolate_partial", count, traj);
    if (rc <= 0) return rc;
    if (c->fused) return set_err(c, KPILQR_ERR_STATE, "kpilqr_fd_interpolate_partial: a KPILQR_FLAG_FUSED context holds no persistent step records (its sweeps read the column store): kpilqr_fd_difference");
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "kpilqr_fd_interpolate_partial before kpilqr_set_keypoints");
    rc = check_complete(c, "kpilqr_fd_interpolate_partial");
    if (rc) return rc;
    KP_HIP(c, hipMemcpyAsync(c->traj_list, traj, (size_t)count * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (linearise_one_pass(c)) {
        rc = ensure_segent(c);
        if (rc) return rc;
        KP_HIP(c, launch_fd_kp_interpolate(c, c->traj_list, count));
        c->last_linearise = c->fd_payload == FdPayload::kp_columns ? "kp_columns_interpolate:subset" : "fd_kp_interpolate:subset";
    } else {
        // job lists: the resident jobs are differenced (whoever they belong to: a kept trajectory's jobs rewrite what its records
        // hold); a payload by entry under KPILQR_FD_INTERP=0: columns -> the listed trajectories' key-point steps; then k_interpolate
        if (c->fd_payload == FdPayload::jobs) KP_HIP(c, launch_fd_difference(c));
        else if (payload_by_entry(c)) {
            if (!c->pay.kpc_valid) { rc = difference_to_kpc(c); if (rc) return rc; }
            rc = ensure_entry_tables(c);
            if (rc) return rc;
            rc = kpc_to_records_of(c, count, traj);
            if (rc) return rc;
        }
        KP_HIP(c, launch_interpolate(c, c->traj_list, count));
        c->last_linearise = "fd_difference+interpolate:subset";
    }
    return wait_unless_pinned(c, traj);
}

// kpilqr_cost_derivs for the listed trajectories
int kpilqr_cost_derivs_partial(kpilqr_ctx *c, int count, const int *traj)
{
    KP_NOT_EMBEDDED(c, "kpilqr_cost_derivs_partial");
    int rc = enter_subset(c, "kpilqr_cost_derivs_partial", count, traj);
    if (rc <= 0) return rc;
    if (c->fused) return set_err(c, KPILQR_ERR_STATE, "kpilqr_cost_derivs_partial: a KPILQR_FLAG_FUSED context holds no persistent step records (its sweeps form the cost derivatives themselves)");
    rc = ensure_rx_buffer(c);
    if (rc) return rc;
    KP_HIP(c, hipMemcpyAsync(c->traj_list, traj, (size_t)count * sizeof(int), hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, launch_cost_derivs(c, c->traj_list, count));
    return wait_unless_pinned(c, traj);
}

// ---- key-point placement on the device for a listed subset: states, placement, and the new lists read back compact -------------------
// All three enter like kpilqr_update_keypoints: the list check of the _partial family, and a view refused in the words of
// everything that allocates.  -> 1: go on | KPILQR_OK: nobody is listed | < 0: refused
static int enter_placement_subset(kpilqr_ctx *c, const char *who, int count, const int *traj)
{
    const int go = enter_subset(c, who, count, traj, Subset::listed_or_view);
    if (go <= 0) return go;
    if (c->is_view) return set_err(c, KPILQR_ERR_STATE, kViewNeverAllocates);
    return 1;
}

int kpilqr_upload_states_partial(kpilqr_ctx *c, int count, const int *traj, const double *X)
{
    KP_NOT_EMBEDDED(c, "kpilqr_upload_states_partial");
    if (count > 0 && !X) return KPILQR_ERR_ARG;
    { const int go = enter_placement_subset(c, "kpilqr_upload_states_partial", count, traj); if (go <= 0) return go; }
    const size_t B = c->d.batch, per = (size_t)c->d.T * c->n;
    { const int rcg = reserve(c, c->X_states, B * per * sizeof(double), kExact, false); if (rcg < 0) return rcg; }
    if (!c->states_given_host) {
        c->states_given_host = (unsigned char *)malloc(B);
        if (!c->states_given_host) return set_err(c, KPILQR_ERR_ALLOC, "host allocation failed");
        memset(c->states_given_host, c->have_states ? 1 : 0, B);
    }
    const int rc = upload_rows(c, count, traj, X, c->X_states, per);
    if (rc) return rc;
    for (int i = 0; i < count; i++) c->states_given_host[traj[i]] = 1;
    return KPILQR_OK;
}

int kpilqr_generate_keypoints_partial(kpilqr_ctx *c, int count, const int *traj, const char *method, int min_N, int max_N,
                                      const double *thresholds, double dt)
{
    KP_NOT_EMBEDDED(c, "kpilqr_generate_keypoints_partial");
    static const char who[] = "kpilqr_generate_keypoints_partial";
    if (!c || !method) return KPILQR_ERR_ARG;
    { const int go = enter_placement_subset(c, who, count, traj); if (go <= 0) return go; }
    int mth = -1;
    int rc = placement_args(c, method, min_N, max_N, thresholds, dt, &mth);
    if (rc) return rc;
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, std::string(who) + " before kpilqr_set_keypoints / kpilqr_generate_keypoints");
    rc = check_complete(c, who);
    if (rc) return rc;
    if (mth != 0 && !c->have_states)
        for (int i = 0; i < count; i++)
            if (!c->states_given_host || !c->states_given_host[traj[i]])
                return set_err(c, KPILQR_ERR_STATE, std::string(who) + ": the states of trajectory " + std::to_string(traj[i]) +
                               " were never uploaded (kpilqr_upload_states / kpilqr_upload_states_partial)");
    rc = ensure_offsets_mirror(c);
    if (rc) return rc;

    // ---- pass 1 over the list, and its counts read back: from here the host knows every size exactly -----------------------------
    const size_t dof = c->d.dof, nlists = (size_t)c->d.batch * dof, nnew = (size_t)count * dof, T = c->d.T, nchunks = (T + 63) / 64;
    const struct { DevMem *buf; size_t bytes; } rows[] = {                // (the whole-batch call's sizes: the two share the buffers)
        {&c->kp_thr, sizeof(double) * dof},
        {&c->kp_mask, sizeof(unsigned long long) * nlists * nchunks},
        {&c->kp_count, sizeof(int) * (2 * nlists + 1)},                   // the compact counts | at nlists: their scan, nnew + 1 offsets
        {&c->X_states, sizeof(double) * c->d.batch * T * c->n},           // set_interval never looks at what it stages from here
    };
    for (const auto &row : rows) { const int rcg = reserve(c, *row.buf, row.bytes, kExact, false); if (rcg < 0) return rcg; }
    int *const counts = (int *)malloc(sizeof(int) * (2 * nnew + 1));
    if (!counts) return set_err(c, KPILQR_ERR_ALLOC, "host allocation failed");
    int *const offs = counts + nnew;
    // (the two arrays are this call's own: whatever was enqueued has read them before they go)
    struct Free { kpilqr_ctx *c; int *p; ~Free() { (void)hipStreamSynchronize(c->stream); free(p); } } guard{c, counts};
    if (thresholds) KP_HIP(c, hipMemcpyAsync(c->kp_thr, thresholds, sizeof(double) * dof, hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, hipMemcpyAsync(c->traj_list, traj, (size_t)count * sizeof(int), hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, launch_kp_flags_listed(c, count, c->traj_list, mth, min_N, max_N, dt, thresholds ? c->kp_thr : nullptr, c->X_states, c->kp_mask, c->kp_count));
    KP_HIP(c, hipMemcpyAsync(counts, c->kp_count, nnew * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    KP_HIP(c, hipStreamSynchronize(c->stream));          // (thresholds and traj, which may be pageable, have been read too)
    const int bad = kp_offsets_from_counts(nnew, (int)T, counts, offs);
    if (bad == 1) return set_err(c, KPILQR_ERR_HIP, std::string(who) + ": implausible key-point counts read back");
    if (bad) return set_err(c, KPILQR_ERR_ARG, std::string(who) + ": more key-point entries than an int counts");

    // ---- pass 3: the bitmasks expanded into the new lists' times, where kpilqr_update_keypoints uploads its caller's -----------
    const int new_entries = offs[nnew];
    { const int rcg = reserve(c, c->kp_upl_times, (size_t)new_entries * sizeof(int), kQuarter, false); if (rcg < 0) return rcg; }
    int *const offs_dev = c->kp_count + nlists;
    KP_HIP(c, hipMemcpyAsync(offs_dev, offs, (nnew + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, launch_kp_fill_listed(c, count, c->kp_mask, offs_dev, c->kp_upl_times));
    // canonical: rows 0 and T-1 are always full and the lists strictly increasing by construction; set_interval: one list for all DoFs
    return install_subset_lists(c, who, count, traj, offs, nullptr, (unsigned char)(kKpCanonical | (mth == 0 ? kKpUniform : 0)));
}

int kpilqr_get_keypoints_partial(kpilqr_ctx *c, int count, const int *traj, int *kp_offsets, int *kp_times, int times_capacity)
{
    KP_NOT_EMBEDDED(c, "kpilqr_get_keypoints_partial");
    if (!c || !kp_offsets) return KPILQR_ERR_ARG;
    {
        const int go = enter_placement_subset(c, "kpilqr_get_keypoints_partial", count, traj);
        if (go < 0) return go;
        if (go == 0) { kp_offsets[0] = 0; return 0; }
    }
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "no key-points set");
    // (ranges may be pending: this reads lists, not payload, and that is when the host needs them.  The mirror answers the size
    // query without the device; behind kpilqr_generate_keypoints it is read back here, once)
    { const int rc = ensure_offsets_mirror(c); if (rc) return rc; }
    const int dof = c->d.dof, *const o = c->kp_offsets_host;
    int at = 0;
    for (int i = 0; i < count; i++)
        for (int d = 0; d < dof; d++) {
            const size_t l = (size_t)traj[i] * dof + d;
            kp_offsets[(size_t)i * dof + d] = at;
            at += o[l + 1] - o[l];
        }
    kp_offsets[(size_t)count * dof] = at;
    if (kp_times) {
        if (at > times_capacity) return set_err(c, KPILQR_ERR_ARG, "kp_times capacity too small");
        int *dst = kp_times;
        const int rc = kp_for_each_run(count, traj, [&](int, int b0, int run) -> int {
            const int e0 = o[(size_t)b0 * dof], len = o[(size_t)(b0 + run) * dof] - e0;
            if (len) KP_HIP(c, hipMemcpyAsync(dst, c->kp_times + e0, (size_t)len * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            dst += len;
            return KPILQR_OK;
        });
        if (rc) return rc;
        KP_HIP(c, hipStreamSynchronize(c->stream));
    }
    return at;
}

// ---- K as FP32: half the bytes of the largest per-iteration download ---------------------------------------------------------------
// K of the rows (traj == nullptr: trajectories 0 .. count-1) is rounded into the context's compact float buffer by ONE launch
// (gains.hip) and leaves with ONE copy; k stays FP64 and is copied as kpilqr_download_gains[_partial] copies it.  The caller has
// checked the list: nothing below rejects an argument.
static int download_gains_f32(kpilqr_ctx *c, int count, const int *traj, float *K32, double *k)
{
    const size_t perK = (size_t)c->d.T * c->n * c->d.m, perk = (size_t)c->d.T * c->d.m;
    if (K32) {
        const int rc = reserve(c, c->K32, (size_t)count * perK * sizeof(float), kExact, false);
        if (rc < 0) return rc;
        if (traj) KP_HIP(c, hipMemcpyAsync(c->traj_list, traj, (size_t)count * sizeof(int), hipMemcpyHostToDevice, c->stream));
        KP_HIP(c, launch_gains_f32(c, traj ? (const int *)c->traj_list : nullptr, count, c->K32));
        KP_HIP(c, hipMemcpyAsync(K32, c->K32, (size_t)count * perK * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    if (k && !traj) KP_HIP(c, hipMemcpyAsync(k, c->k, (size_t)count * perk * 8, hipMemcpyDeviceToHost, c->stream));
    if (k && traj) {
        const int rc = kp_for_each_run(count, traj, [&](int i, int b0, int run) -> int {
            KP_HIP(c, hipMemcpyAsync(k + (size_t)i * perk, c->k + (size_t)b0 * perk, (size_t)run * perk * 8, hipMemcpyDeviceToHost, c->stream));
            return KPILQR_OK;
        });
        if (rc) return rc;
    }
    return K32 ? wait_unless_pinned(c, traj) : KPILQR_OK;      // (traj was copied to the device for the rounding launch; nullptr counts as pinned)
}

int kpilqr_download_gains_f32(kpilqr_ctx *c, float *K32, double *k)
{
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (c->is_view) return set_err(c, KPILQR_ERR_STATE, "kpilqr_download_gains_f32: not through a view of a trajectory range");
    if (c->embed.on) return download_embedded_gains(c, K32, true, k);
    return download_gains_f32(c, c->d.batch, nullptr, K32, k);
}

int kpilqr_download_gains_f32_partial(kpilqr_ctx *c, int count, const int *traj, float *K32, double *k)
{
    KP_NOT_EMBEDDED(c, "kpilqr_download_gains_f32_partial");
    const int go = enter_subset(c, "kpilqr_download_gains_f32_partial", count, traj);
    if (go <= 0) return go;
    return download_gains_f32(c, count, traj, K32, k);
}

// as launch_backward_family
static hipError_t launch_forward_family(Ctx *lc, double *U_dev)
{
    switch (lc->fwd_family) {
    case Family::t1: return launch_forward_mfma(lc, U_dev);
    case Family::tiled: return launch_forward_tiled(lc, U_dev);
    case Family::wide: return launch_forward_wide(lc, U_dev);
    default: return launch_forward_generic(lc, U_dev);
    }
}

static int run_forward(kpilqr_ctx *c, double *U_dev)
{
    c->last_width[1] = -1;
    if (c->fused) {
        int rc = check_fused(c);
        if (rc) return rc;
        if (union_route(c)) {
            rc = prepare_union(c);
            if (rc) return rc;
            kpilqr_ctx v;
            make_union_view(c, &v);
            FusedLaunch plan = plan_forward_fused(&v);
            plan.uni_on_union = true;
            c->last_fwd = plan;
            if (!plan.rxc) { rc = ensure_rx_buffer(c); if (rc) return rc; }
            KP_HIP(c, launch_forward_fused(&v, plan, U_dev));
            c->last_fwd.fwd_ran = true;
            return KPILQR_OK;
        }
        rc = ensure_kpc(c);
        if (rc) return rc;
        rc = ensure_kps(c);
        if (rc) return rc;
        const FusedLaunch plan = c->last_fwd = plan_forward_fused(c);
        if (!plan.rxc) { rc = ensure_rx_buffer(c); if (rc) return rc; }       // (as in run_backward)
        // kpc: differenced explicitly, or left behind by the raw backward sweep of this payload
        if (!c->pay.kpc_valid && !c->pay.kpc_touched) { rc = difference_to_kpc(c); if (rc) return rc; }
        if (c->pay.kpc_valid) { rc = slopes_for_kpc(c); if (rc) return rc; }       // (behind a raw backward sweep: its launch sequence made them)
        KP_HIP(c, launch_forward_fused(c, plan, U_dev));
        c->last_fwd.fwd_ran = true;
        return KPILQR_OK;
    }
    c->last_fwd = FusedLaunch{};
    if (c->tiled_a6) { const int rc = ensure_rx_buffer(c); if (rc) return rc; }
    KP_HIP(c, launch_forward_family(c, U_dev));
    c->last_fwd.fwd_ran = true;
    return KPILQR_OK;
}

int kpilqr_forward_linear(kpilqr_ctx *c, const double *alphas, double *cost_pred, double *U_alpha)
{
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    const size_t B = c->d.batch, T = c->d.T, m = c->d.m, na = c->d.n_alpha;
    if (alphas) KP_HIP(c, hipMemcpyAsync(c->alphas, alphas, na * 8, hipMemcpyHostToDevice, c->stream));
    double *U_dev = nullptr;
    if (U_alpha) {
        int rc = ensure_stage(c, B * na * T * m * 8);
        if (rc) return rc;
        U_dev = c->stage;
    }
    int rc = run_forward(c, U_dev);
    if (rc) return rc;
    if (cost_pred) KP_HIP(c, hipMemcpyAsync(cost_pred, c->cost_pred, B * na * 8, hipMemcpyDeviceToHost, c->stream));
    if (U_alpha && c->embed.on) {          // the controls of the real block, compact, by the launch that extracts k
        const size_t om = caller_m(c);
        { const int rcs = ensure_emb_stage(c, B * na * T * om * 8); if (rcs) return rcs; }
        KP_HIP(c, launch_extract_gains(c, (int)B, (long long)(na * T), 1, (int)om, 1, (int)m, 1, 0, U_dev, c->emb_stage.p, false));
        KP_HIP(c, hipMemcpyAsync(U_alpha, c->emb_stage.p, B * na * T * om * 8, hipMemcpyDeviceToHost, c->stream));
        return KPILQR_OK;
    }
    if (U_alpha) KP_HIP(c, hipMemcpyAsync(U_alpha, U_dev, B * na * T * m * 8, hipMemcpyDeviceToHost, c->stream));
    return KPILQR_OK;
}

// ---- whole iteration ------------------------------------------------------------------------------
int kpilqr_iterate(kpilqr_ctx *c, const double *lambda, int pd_check_stride, const double *alphas)
{
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "kpilqr_iterate before kpilqr_set_keypoints");
    if (pd_check_stride < 1) return set_err(c, KPILQR_ERR_ARG, "pd_check_stride must be >= 1");
    { const int rcp = check_complete(c, "kpilqr_iterate"); if (rcp) return rcp; }
    { const int rcl = check_embedded_lambda(c, "kpilqr_iterate", lambda); if (rcl) return rcl; }
    if (lambda) KP_HIP(c, hipMemcpyAsync(c->lambda, lambda, (size_t)c->d.batch * 8, hipMemcpyHostToDevice, c->stream));
    if (alphas) KP_HIP(c, hipMemcpyAsync(c->alphas, alphas, (size_t)c->d.n_alpha * 8, hipMemcpyHostToDevice, c->stream));
    if (!c->fused) {              // the fused sweeps difference (or read kpc), interpolate A, B and form l_* themselves
        { const int rcl = linearise(c); if (rcl) return rcl; }
        if (!c->tiled_a6) { const int rcx = ensure_rx_buffer(c); if (rcx) return rcx; KP_HIP(c, launch_cost_derivs(c)); }      // tiled + flag: l_* are formed inside the sweeps
    }
    else c->last_linearise = union_route(c) ? "kp_union" : "in_sweep";
    c->retry_attempts = retry_attempts_for(c, lambda, c->d.batch);
    int rc = run_backward(c, pd_check_stride);
    if (rc) return rc;
    return run_forward(c, nullptr);
}

// ---- the sweeps over a listed subset of the batch (include/kpilqr.h, "Sweeps of a subset") ---------------------------------------------
// A copy of the context for the launchers, as make_view's: d.batch is the list's length -- the launch width, by which the launchers and
// the fused plans choose what only arranges waves -- sweep_list the device copy of the list; every per-trajectory pointer stays the
// context's, block i finds its trajectory through the list.  n_simd stays the chip's: a listed launch has it to itself.  Made AFTER
// everything that may allocate: it borrows the pointers.
static void make_list_view(const kpilqr_ctx *c, int count, kpilqr_ctx *v)
{
    *v = *c;
    v->is_view = true;
    v->own_stream = false;
    v->d.batch = count;
    v->sweep_list = c->traj_list;
}

// the compact staging regions of a listed call with `count` rows, inside sweep_stage
struct SweepStage { double *lambda, *delta_J, *cost_pred; int *status; };
static int sweep_stage_of(kpilqr_ctx *c, int count, SweepStage *s)
{
    const size_t na = c->d.n_alpha, n8 = (size_t)count * 8;
    const int rc = reserve(c, c->sweep_stage, n8 * (2 + na) + (size_t)count * 4, kExact, false);
    if (rc < 0) return rc;
    char *p = c->sweep_stage;
    s->lambda = (double *)p; s->delta_J = (double *)(p + n8); s->cost_pred = (double *)(p + 2 * n8); s->status = (int *)(p + n8 * (2 + na));
    return KPILQR_OK;
}

// everything a listed sweep refuses, before anything is enqueued or changed; -> 1: go on, as enter_subset
static int enter_sweep_subset(kpilqr_ctx *c, const char *who, int count, const int *traj, bool backward, int pd_check_stride)
{
    const int go = enter_subset(c, who, count, traj);
    if (go <= 0) return go;
    if (backward && pd_check_stride < 1) return set_err(c, KPILQR_ERR_ARG, "pd_check_stride must be >= 1");
    { const int rcp = check_complete(c, who); if (rcp) return rcp; }
    if (c->fused) { const int rcf = check_fused(c); if (rcf) return rcf; }
    return 1;
}

// Fused contexts: a listed sweep reads the column store and never differences inside the sweep; a store that is not valid is
// differenced for the whole batch first (kpilqr_fd_difference's launch, with the slopes per-DoF lists need) and is then valid for everybody.
static int columns_for_listed_sweep(kpilqr_ctx *c)
{
    int rc = ensure_kpc(c);
    if (rc) return rc;
    rc = ensure_kps(c);
    if (rc) return rc;
    if (!c->pay.kpc_valid) { rc = difference_to_kpc(c); if (rc) return rc; }
    if (c->pay.kpc_valid) { rc = slopes_for_kpc(c); if (rc) return rc; }
    return KPILQR_OK;
}

// The launches of a listed backward / forward sweep on the list view v -- of the context (make_list_view) or of a chunk of a streamed
// iteration (make_chunk_list_view) -- behind everything that may allocate; c, the context, records what ran.
static int launch_backward_listed(kpilqr_ctx *c, kpilqr_ctx *v, int pd_stride)
{
    c->last_width[0] = v->d.batch;
    if (c->fused) {
        const FusedLaunch plan = c->last_bwd = plan_backward_fused(v, false);
        return sweep_attempts(c, v, [&] { return launch_backward_fused(v, plan, pd_stride); });
    }
    c->last_bwd = FusedLaunch{};
    return sweep_attempts(c, v, [&] { return launch_backward_family(v, pd_stride); });
}

static int launch_forward_listed(kpilqr_ctx *c, kpilqr_ctx *v, double *U_dev)
{
    c->last_width[1] = v->d.batch;
    if (c->fused) {
        const FusedLaunch plan = c->last_fwd = plan_forward_fused(v);
        KP_HIP(c, launch_forward_fused(v, plan, U_dev));
    } else {
        c->last_fwd = FusedLaunch{};
        KP_HIP(c, launch_forward_family(v, U_dev));
    }
    c->last_fwd.fwd_ran = true;
    return KPILQR_OK;
}

// the broadcast copy of constant residual Jacobians, where a listed sweep streams r_x (a plan's rxc does not depend on the launch width)
static int rx_buffer_for_listed_sweep(kpilqr_ctx *c, bool backward)
{
    const bool streams_rx = c->fused ? !(backward ? plan_backward_fused(c, false) : plan_forward_fused(c)).rxc : c->tiled_a6;
    return streams_rx ? ensure_rx_buffer(c) : KPILQR_OK;
}

// the list is on the device (traj_list) and checked
static int run_backward_listed(kpilqr_ctx *c, int count, int pd_stride)
{
    if (c->fused) { const int rc = columns_for_listed_sweep(c); if (rc) return rc; }
    { const int rc = rx_buffer_for_listed_sweep(c, true); if (rc) return rc; }
    kpilqr_ctx v;
    make_list_view(c, count, &v);
    return launch_backward_listed(c, &v, pd_stride);
}

static int run_forward_listed(kpilqr_ctx *c, int count, double *U_dev)
{
    if (c->fused) { const int rc = columns_for_listed_sweep(c); if (rc) return rc; }
    { const int rc = rx_buffer_for_listed_sweep(c, false); if (rc) return rc; }
    kpilqr_ctx v;
    make_list_view(c, count, &v);
    return launch_forward_listed(c, &v, U_dev);
}

// the list and the compact lambdas to the device; the lambdas placed by ONE launch
static int listed_inputs(kpilqr_ctx *c, int count, const int *traj, const double *lambda, const SweepStage &st)
{
    KP_HIP(c, hipMemcpyAsync(c->traj_list, traj, (size_t)count * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (lambda) {
        KP_HIP(c, hipMemcpyAsync(st.lambda, lambda, (size_t)count * 8, hipMemcpyHostToDevice, c->stream));
        KP_HIP(c, launch_rows_in(c->stream, c->traj_list, count, 1, st.lambda, c->lambda));
    }
    return KPILQR_OK;
}

static int backward_listed(kpilqr_ctx *c, int count, const int *traj, const double *lambda, int pd_check_stride, int *status, double *delta_J)
{
    SweepStage st;
    int rc = sweep_stage_of(c, count, &st);
    if (rc) return rc;
    rc = listed_inputs(c, count, traj, lambda, st);
    if (rc) return rc;
    c->retry_attempts = retry_attempts_for(c, lambda, (size_t)count);
    rc = run_backward_listed(c, count, pd_check_stride);
    if (rc) return rc;
    if (status) {
        KP_HIP(c, launch_rows_out(c->stream, c->traj_list, count, 1, (const int *)c->status, st.status));
        KP_HIP(c, hipMemcpyAsync(status, st.status, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if (delta_J) {
        KP_HIP(c, launch_rows_out(c->stream, c->traj_list, count, 2, (const double *)c->delta_J, st.delta_J));
        KP_HIP(c, hipMemcpyAsync(delta_J, st.delta_J, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
    }
    return KPILQR_OK;
}

static int forward_listed(kpilqr_ctx *c, int count, const int *traj, bool list_resident, const double *alphas, double *cost_pred, double *U_alpha)
{
    const size_t B = c->d.batch, T = c->d.T, m = c->d.m, na = c->d.n_alpha;
    SweepStage st;
    int rc = sweep_stage_of(c, count, &st);
    if (rc) return rc;
    if (!list_resident) KP_HIP(c, hipMemcpyAsync(c->traj_list, traj, (size_t)count * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (alphas) KP_HIP(c, hipMemcpyAsync(c->alphas, alphas, na * 8, hipMemcpyHostToDevice, c->stream));
    double *U_dev = nullptr;
    if (U_alpha) {              // (debug output: the sweep writes a trajectory's controls at its own place of a whole-batch staging area)
        rc = ensure_stage(c, B * na * T * m * 8);
        if (rc) return rc;
        U_dev = c->stage;
    }
    rc = run_forward_listed(c, count, U_dev);
    if (rc) return rc;
    if (cost_pred) {
        KP_HIP(c, launch_rows_out(c->stream, c->traj_list, count, 2 * (int)na, (const double *)c->cost_pred, st.cost_pred));
        KP_HIP(c, hipMemcpyAsync(cost_pred, st.cost_pred, (size_t)count * na * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (U_alpha) {
        const size_t per = na * T * m;
        rc = kp_for_each_run(count, traj, [&](int i, int b0, int run) -> int {
            KP_HIP(c, hipMemcpyAsync(U_alpha + (size_t)i * per, U_dev + (size_t)b0 * per, (size_t)run * per * 8, hipMemcpyDeviceToHost, c->stream));
            return KPILQR_OK;
        });
        if (rc) return rc;
    }
    return KPILQR_OK;
}

int kpilqr_backward_partial(kpilqr_ctx *c, int count, const int *traj, const double *lambda, int pd_check_stride, int *status, double *delta_J)
{
    KP_NOT_EMBEDDED(c, "kpilqr_backward_partial");
    const int go = enter_sweep_subset(c, "kpilqr_backward_partial", count, traj, true, pd_check_stride);
    if (go <= 0) return go;
    const int rc = backward_listed(c, count, traj, lambda, pd_check_stride, status, delta_J);
    return rc ? rc : wait_unless_pinned(c, traj);
}

int kpilqr_forward_linear_partial(kpilqr_ctx *c, int count, const int *traj, const double *alphas, double *cost_pred, double *U_alpha)
{
    KP_NOT_EMBEDDED(c, "kpilqr_forward_linear_partial");
    const int go = enter_sweep_subset(c, "kpilqr_forward_linear_partial", count, traj, false, 1);
    if (go <= 0) return go;
    const int rc = forward_listed(c, count, traj, false, alphas, cost_pred, U_alpha);
    return rc ? rc : wait_unless_pinned(c, traj);
}

// kpilqr_iterate for the listed trajectories.  A context with records: kpilqr_fd_interpolate_partial, kpilqr_cost_derivs_partial (not
// where the tiled sweeps form the cost derivatives themselves), then the two sweeps; a fused context: the two sweeps.
int kpilqr_iterate_partial(kpilqr_ctx *c, int count, const int *traj, const double *lambda, int pd_check_stride, const double *alphas)
{
    KP_NOT_EMBEDDED(c, "kpilqr_iterate_partial");
    const int go = enter_sweep_subset(c, "kpilqr_iterate_partial", count, traj, true, pd_check_stride);
    if (go <= 0) return go;
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "kpilqr_iterate_partial before kpilqr_set_keypoints");
    if (!c->fused) {
        int rcl = kpilqr_fd_interpolate_partial(c, count, traj);
        if (rcl) return rcl;
        if (!c->tiled_a6) { rcl = kpilqr_cost_derivs_partial(c, count, traj); if (rcl) return rcl; }
    }
    else c->last_linearise = "in_sweep:subset";
    int rc = backward_listed(c, count, traj, lambda, pd_check_stride, nullptr, nullptr);
    if (rc) return rc;
    rc = forward_listed(c, count, traj, true, alphas, nullptr, nullptr);
    return rc ? rc : wait_unless_pinned(c, traj);
}

// ---- whole iteration, pipelined over chunks of trajectories ------------------------------------------------------------
static int pipe_setup(kpilqr_ctx *c)
{
    if (c->pipe_ready) return KPILQR_OK;
    for (int i = 0; i < Ctx::kPipeStreams; i++) {
        KP_HIP(c, hipStreamCreateWithFlags(&c->pipe_stream[i], hipStreamNonBlocking));
        KP_HIP(c, hipEventCreateWithFlags(&c->pipe_done[i], hipEventDisableTiming));
    }
    KP_HIP(c, hipEventCreateWithFlags(&c->pipe_in, hipEventDisableTiming));
    c->pipe_ready = true;
    return KPILQR_OK;
}

// doubles per trajectory of the arrays a chunk moves: the one place that spells them (views, staging regions, uploads, downloads)
struct RowSizes { size_t r, r_x, r_u, u_nom, K, k; };
static RowSizes row_sizes(const kpilqr_ctx *c)
{
    const size_t T = c->d.T, n = c->n, m = c->d.m, nr = c->d.nr;
    return {(T + 1) * nr, (T + 1) * nr * n, (T + 1) * nr * m, T * m, T * n * m, T * m};
}

// first trajectory of chunk ch of nchunks (ch == nchunks: the batch's end)
static int chunk_first(int B, int ch, int nchunks) { return (int)((long long)B * ch / nchunks); }

// A view of trajectories [b0, b0+nb) of context c on stream s: every per-trajectory pointer shifted, so the ordinary
// launchers run unchanged on the chunk.  n_simd is the chunk's SHARE of the chip: the launchers pick their wave
// organisation (wave pairs / triples per trajectory) as if the whole batch were in flight, which it is.  Where the host knows the
// lists the view carries its trajectories' entry range, [fdk_first, fdk_first + kp_view_entries): the one place that reads it.
static void make_view(const kpilqr_ctx *c, int b0, int nb, hipStream_t s, kpilqr_ctx *v)
{
    *v = *c;
    v->is_view = true;             // it borrows the context's buffers: reserve() refuses to grow one through it
    const size_t T = c->d.T, na = c->d.n_alpha, dof = c->d.dof, o = (size_t)b0;
    const RowSizes per = row_sizes(c);
    v->d.batch = nb; v->stream = s; v->own_stream = false;
    if (v->rec) v->rec.shift(o * T * c->L.stride);
    v->K.shift(o * per.K); v->k.shift(o * per.k);
    v->r.shift(o * per.r); v->r_x.shift(o * per.r_x); v->r_u.shift(o * per.r_u);
    v->u_nom.shift(o * per.u_nom); v->lambda.shift(o); v->cost_pred.shift(o * na); v->delta_J.shift(o); v->traj_cost.shift(o); v->status.shift(o);
    v->attempts.shift(o); v->gate.shift(o);
    v->segmap.shift(o * dof * T); v->kp_offsets.shift(o * dof);
    if (v->segent) v->segent.shift(o * dof * T);
    if (c->kp_traj_first_host) { v->fdk_first = c->kp_traj_first_host[b0]; v->kp_view_entries = c->kp_traj_first_host[b0 + nb] - v->fdk_first; }
    long long share = (long long)c->n_simd * nb / c->d.batch;
    v->n_simd = share < 4 ? 4 : (int)share;
}

// A list of trajectories (strictly increasing, within [0, batch)) that a streamed iteration follows, and the walk over it: chunks and
// list both increase, so a chunk's share is the slice the cursor passes on its way to the chunk's end.
struct StreamList {
    bool listed = false;
    int count = 0, pos = 0;        // pos: first entry no chunk has taken yet
    const int *traj = nullptr;
    void slice_below(int b1, int *i0, int *i1) { *i0 = pos; while (pos < count && traj[pos] < b1) pos++; *i1 = pos; }
};

// The FD payload a streamed iteration brings, decided once (at the "one FD payload per iteration" refusal of stream_check)
enum class StreamPayload { none, jobs, kp_ordered, columns, columns_f32 };

// A streamed iteration, resolved: what the six entry points ask for (they fill the first group), what stream_check decides about the
// payload, and where stream_prepare found the device side of it.  The three kinds by key-point entry (kp_ordered, columns,
// columns_f32) differ in the fields below and in nothing else: a chunk copies ONE contiguous range of `rec` bytes per entry from
// `src` to `land` at its own first entry, and one launch may follow (stream_chunk_payload).
struct StreamCall {
    const kpilqr_stream_io *io = nullptr;
    int pd_check_stride = 0, nchunks = 0;
    float *K32 = nullptr;              // kpilqr_iterate_streamed2: K rounded to FP32 instead of io->K
    StreamList gains;                  // kpilqr_iterate_streamed2: K / K32 / k of those rows alone, compact
    const float *kcols32 = nullptr;    // kpilqr_iterate_streamed3: the ENCODED FP32 key-point columns (kpilqr_upload_kp_columns_f32) for a payload
    StreamList rows;                   // kpilqr_iterate_streamed4: the inputs (payload, r, r_x, r_u, u_nom) of those trajectories alone, compact; read during the call only
    StreamList sweep;                  // kpilqr_iterate_streamed5: the linearisation and the sweeps of those trajectories alone; lambda, cost_pred, delta_J, status compact
    const float *rx32 = nullptr, *ru32 = nullptr;      // kpilqr_iterate_streamed6: r_x / r_u as FP32 (kpilqr_upload_residual_jacobians_f32) instead of io->r_x / io->r_u; compact with `rows`
    // stream_check
    StreamPayload kind = StreamPayload::none;
    const char *src = nullptr;         // by entry: the host source ...
    size_t rec = 0;                    // ... and its bytes per entry (the record stride | 3n doubles | 3n floats)
    // stream_prepare
    kpilqr_fd_layout L{};              // jobs: the slab's layout
    char *land = nullptr;              // by entry: device base a chunk's range is copied to (fdk_dev | kpc | kpc32; FP64 of a list: rows_stage[kRowsPayload])
    void *place = nullptr;             // FP64 of a list: where launch_rows_in_entries moves the listed ranges from `land` (fdk_dev | kpc)
    const int *ulist = nullptr, *ufirst = nullptr;      // rows: the list and the per-trajectory first entries on the device (its ring slot)
    int uslot = 0;
    const int *slist = nullptr;        // sweep: the list on the device (its ring slot)
    int sslot = 0;
    bool k_up = false, k_down = false; // copies by kernel (KPILQR_PIPE_COPY)
    StreamCall(const kpilqr_stream_io *io_, int stride, int chunks) : io(io_), pd_check_stride(stride), nchunks(chunks) {}
    bool by_entry() const { return kind != StreamPayload::none && kind != StreamPayload::jobs; }
    hipError_t h2d(void *dst, const void *from, size_t bytes, hipStream_t s) const      // a chunk's inputs: by SDMA, or by the copy kernel
    {
        return k_up ? launch_copy_in(s, dst, from, bytes) : hipMemcpyAsync(dst, from, bytes, hipMemcpyHostToDevice, s);
    }
};

// The list of a streamed iteration on the device, before the chunks are cut: reserved and filled on the CONTEXT (a view never
// allocates), on the context's stream ahead of pipe_in.  A list equal to the one the device copy holds is not uploaded again, so
// consecutive calls keep overlapping; a different one first orders the context's stream behind the chunks still reading the old one.
static int pipe_list_bind(kpilqr_ctx *c, const StreamList &g)
{
    if (!g.listed || g.count == 0) return KPILQR_OK;
    const size_t B = c->d.batch;
    { const int rc = reserve(c, c->pipe_list, B * sizeof(int), kExact, false); if (rc < 0) return rc; }
    if (!c->pipe_list_host) {
        const hipError_t e = hipHostMalloc((void **)&c->pipe_list_host, B * sizeof(int), hipHostMallocDefault);
        if (e != hipSuccess) { c->pipe_list_host = nullptr; return set_err(c, KPILQR_ERR_ALLOC, std::string("hipHostMalloc failed: ") + hipGetErrorString(e)); }
    }
    if (!c->pipe_list_up) KP_HIP(c, hipEventCreateWithFlags(&c->pipe_list_up, hipEventDisableTiming));
    if (c->pipe_list_count == g.count && memcmp(c->pipe_list_host, g.traj, sizeof(int) * (size_t)g.count) == 0) return KPILQR_OK;
    { const int rc = join_pipeline(c); if (rc) return rc; }
    if (c->pipe_list_count >= 0) KP_HIP(c, hipEventSynchronize(c->pipe_list_up));      // the mirror's last upload has read it
    memcpy(c->pipe_list_host, g.traj, sizeof(int) * (size_t)g.count);
    c->pipe_list_count = g.count;
    KP_HIP(c, hipMemcpyAsync(c->pipe_list, c->pipe_list_host, sizeof(int) * (size_t)g.count, hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, hipEventRecord(c->pipe_list_up, c->stream));
    return KPILQR_OK;
}

// A buffer that grows is freed: nothing in flight may still read it.  If one of `needs` (buffer, bytes) would grow, the pipeline is
// joined and the host waits for every chunk stream; the caller's reserve() then waits for the context's stream, as always.
static int quiesce_for_growth(kpilqr_ctx *c, std::initializer_list<std::pair<const DevMem *, size_t>> needs)
{
    bool grows = false;
    for (const auto &nd : needs) grows = grows || would_grow(*nd.first, nd.second);
    if (!grows) return KPILQR_OK;
    { const int rc = join_pipeline(c); if (rc) return rc; }
    for (int i = 0; i < Ctx::kPipeStreams; i++) KP_HIP(c, hipStreamSynchronize(c->pipe_stream[i]));
    return KPILQR_OK;
}

// The ring slot of a listed call, before the chunks are cut: the list and, per trajectory, the first entry of its payload inside the
// staging region (-1: not listed) into the slot's pinned mirror, uploaded on the context's stream ahead of pipe_in.  The slot was
// last used kRowsRing calls ago: the wait for its upload is over long since, and the context's stream is ordered behind the chunks
// that read its device copy -- no wait concerns the iteration in flight.  -> *slot_out
static int rows_list_bind(kpilqr_ctx *c, const StreamList &u, int nchunks, bool by_entry, int *slot_out)
{
    const int B = c->d.batch, slot = c->rows_next;
    const size_t per_slot = 2 * (size_t)B;
    if (!c->rows_list_host) {
        { const int rc = reserve(c, c->rows_list, Ctx::kRowsRing * per_slot * sizeof(int), kExact, false); if (rc < 0) return rc; }
        const hipError_t e = hipHostMalloc((void **)&c->rows_list_host, Ctx::kRowsRing * per_slot * sizeof(int), hipHostMallocDefault);
        if (e != hipSuccess) { c->rows_list_host = nullptr; return set_err(c, KPILQR_ERR_ALLOC, std::string("hipHostMalloc failed: ") + hipGetErrorString(e)); }
    }
    if (!c->rows_up[slot]) {
        KP_HIP(c, hipEventCreateWithFlags(&c->rows_up[slot], hipEventDisableTiming));
        for (int i = 0; i < Ctx::kPipeStreams; i++) KP_HIP(c, hipEventCreateWithFlags(&c->rows_read[slot][i], hipEventDisableTiming));
    } else {
        KP_HIP(c, hipEventSynchronize(c->rows_up[slot]));
    }
    for (int i = 0; i < Ctx::kPipeStreams; i++)
        if (c->rows_read_set[slot][i]) { KP_HIP(c, hipStreamWaitEvent(c->stream, c->rows_read[slot][i], 0)); c->rows_read_set[slot][i] = false; }
    int *const list = c->rows_list_host + slot * per_slot, *const first = list + B;
    memcpy(list, u.traj, sizeof(int) * (size_t)u.count);
    for (int b = 0; b < B; b++) first[b] = -1;
    if (by_entry) {
        // a chunk's listed entries sit back to back from the chunk's own first entry on
        for (int ch = 0, i = 0; ch < nchunks; ch++) {
            const int b1 = chunk_first(B, ch + 1, nchunks);
            int at = c->kp_traj_first_host[chunk_first(B, ch, nchunks)];
            for (; i < u.count && u.traj[i] < b1; i++) {
                first[u.traj[i]] = at;
                at += c->kp_traj_first_host[u.traj[i] + 1] - c->kp_traj_first_host[u.traj[i]];
            }
        }
    }
    KP_HIP(c, hipMemcpyAsync((int *)c->rows_list + slot * per_slot, list, per_slot * sizeof(int), hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, hipEventRecord(c->rows_up[slot], c->stream));
    c->rows_next = (slot + 1) % Ctx::kRowsRing;
    *slot_out = slot;
    return KPILQR_OK;
}

// The same for the sweep list of kpilqr_iterate_streamed5: the list alone, [batch] ints per slot of its own ring.  -> *slot_out
static int sweep_list_bind(kpilqr_ctx *c, const StreamList &w, int *slot_out)
{
    const int slot = c->sweep_next;
    const size_t per_slot = (size_t)c->d.batch;
    if (!c->sweep_ring_host) {
        { const int rc = reserve(c, c->sweep_ring, Ctx::kRowsRing * per_slot * sizeof(int), kExact, false); if (rc < 0) return rc; }
        const hipError_t e = hipHostMalloc((void **)&c->sweep_ring_host, Ctx::kRowsRing * per_slot * sizeof(int), hipHostMallocDefault);
        if (e != hipSuccess) { c->sweep_ring_host = nullptr; return set_err(c, KPILQR_ERR_ALLOC, std::string("hipHostMalloc failed: ") + hipGetErrorString(e)); }
    }
    if (!c->sweep_up[slot]) {
        KP_HIP(c, hipEventCreateWithFlags(&c->sweep_up[slot], hipEventDisableTiming));
        for (int i = 0; i < Ctx::kPipeStreams; i++) KP_HIP(c, hipEventCreateWithFlags(&c->sweep_read[slot][i], hipEventDisableTiming));
    } else {
        KP_HIP(c, hipEventSynchronize(c->sweep_up[slot]));
    }
    for (int i = 0; i < Ctx::kPipeStreams; i++)
        if (c->sweep_read_set[slot][i]) { KP_HIP(c, hipStreamWaitEvent(c->stream, c->sweep_read[slot][i], 0)); c->sweep_read_set[slot][i] = false; }
    int *const list = c->sweep_ring_host + slot * per_slot;
    memcpy(list, w.traj, sizeof(int) * (size_t)w.count);
    KP_HIP(c, hipMemcpyAsync((int *)c->sweep_ring + slot * per_slot, list, sizeof(int) * (size_t)w.count, hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, hipEventRecord(c->sweep_up[slot], c->stream));
    c->sweep_next = (slot + 1) % Ctx::kRowsRing;
    *slot_out = slot;
    return KPILQR_OK;
}

// Phase 1 of a streamed iteration -- EVERY refusal, before a single operation is enqueued or the context is changed: nothing here
// writes to *c but set_err (and the join ahead of check_complete, which orders streams and changes no derived state).  It decides the
// payload's kind, and for job lists returns in *sig the FNV-1a hash of what decides where a chunk's payload lands.
static int stream_check(kpilqr_ctx *c, StreamCall *call, unsigned long long *sig)
{
    const kpilqr_stream_io *io = call->io;
    const StreamList &u = call->rows, &g = call->gains;
    const float *kcols32 = call->kcols32;
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "kpilqr_iterate_streamed before kpilqr_set_keypoints");
    if (call->pd_check_stride < 1) return set_err(c, KPILQR_ERR_ARG, "pd_check_stride must be >= 1");
    // (a whole new payload completes the resident one; without it the pending ranges of kpilqr_update_keypoints would be read)
    if (!io->fd_slab && !io->fd_kp_slab && !io->kp_columns && !kcols32) {
        if (c->n_pending) { const int rcj = join_pipeline(c); if (rcj) return rcj; }
        const int rcp = check_complete(c, "kpilqr_iterate_streamed without a new payload"); if (rcp) return rcp;
    }
    const int B = c->d.batch;
    if (u.listed && !kp_traj_list_ok(B, u.count, u.traj))
        return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed4: upload_traj must be strictly increasing and within [0, batch)");
    if (io->fd_slab && (io->njobs < 1 || !io->traj_job_first || (io->nnom > 0 && !io->traj_nom_first)))
        return set_err(c, KPILQR_ERR_ARG, "streamed FD payload needs the per-trajectory job / nominal-row offsets");
    if ((io->fd_slab != nullptr) + (io->fd_kp_slab != nullptr) + (io->kp_columns != nullptr) + (kcols32 != nullptr) > 1)
        return set_err(c, KPILQR_ERR_ARG, "one FD payload per iteration: job lists OR key-point ordered OR key-point columns (FP64 OR FP32)");
    const size_t n3 = (size_t)3 * c->n;
    kpilqr_fdkp_layout LK{};
    fdkp_layout(c->n, 0, &LK);
    if (io->fd_slab) call->kind = StreamPayload::jobs;
    if (io->fd_kp_slab) { call->kind = StreamPayload::kp_ordered; call->src = (const char *)io->fd_kp_slab; call->rec = LK.entry_stride; }
    if (io->kp_columns) { call->kind = StreamPayload::columns; call->src = (const char *)io->kp_columns; call->rec = n3 * sizeof(double); }
    if (kcols32) { call->kind = StreamPayload::columns_f32; call->src = (const char *)kcols32; call->rec = n3 * sizeof(float); }
    if (call->by_entry()) {
        if (!c->kp_traj_first_host || c->kp_total_host < 0)
            return set_err(c, KPILQR_ERR_STATE, "streamed key-point ordered payload: the lists must be known to the host (kpilqr_set_keypoints, or kpilqr_get_keypoints after generating them)");
        if (!u.listed && io->entries != c->kp_total_host) return set_err(c, KPILQR_ERR_ARG, "fd_kp_slab / kp_columns / kp_columns32: `entries` is not the number of key-point entries");
    }
    // inputs that follow a list (kpilqr_iterate_streamed4 with upload_traj): the list itself has been checked, and with a by-entry
    // payload the host knows the lists
    static const std::string w("kpilqr_iterate_streamed4");
    if (u.listed && io->fd_slab) return set_err(c, KPILQR_ERR_ARG, w + ": io.fd_slab with upload_traj (job lists carry their own trajectory indices: out of scope)");
    if (u.listed && call->by_entry()) {
        long long sum = 0;
        for (int i = 0; i < u.count; i++) sum += c->kp_traj_first_host[u.traj[i] + 1] - c->kp_traj_first_host[u.traj[i]];
        if (io->entries != sum) return set_err(c, KPILQR_ERR_ARG, w + ": `entries` is not the number of key-point entries of the listed trajectories");
        // the trajectories that are not listed keep their payload: it has to be there, whole, and of the kind that arrives
        const FdPayload kind = io->fd_kp_slab ? FdPayload::kp_ordered : FdPayload::kp_columns;
        const bool resident = c->fd_payload == kind && (kind == FdPayload::kp_ordered || c->pay.kpc_valid || c->n_pending > 0);
        if (!resident)
            return set_err(c, KPILQR_ERR_STATE, w + ": a payload with upload_traj, but the context holds no complete resident payload of the same kind "
                                                    "(key-point ordered records / key-point columns) for the trajectories that are not listed");
        if (io->fd_kp_slab && memcmp(&io->eps, &c->eps, sizeof(double)) != 0)
            return set_err(c, KPILQR_ERR_ARG, w + ": eps differs from the resident payload's (a context has one eps)");
        // ranges pending since kpilqr_update_keypoints: the list has to bring every one of them (both lists increase)
        for (int p = 0, i = 0; p < c->n_pending; p++) {
            const int b = c->kp_pending_host[p];
            while (i < u.count && u.traj[i] < b) i++;
            if (i == u.count || u.traj[i] != b)
                return set_err(c, KPILQR_ERR_STATE, w + ": the payload of trajectory " + std::to_string(b) + " is pending since kpilqr_update_keypoints "
                                                        "and upload_traj does not list it");
        }
    }
    // sweeps that follow a list (kpilqr_iterate_streamed5 with sweep_traj): a re-linearised trajectory is an active one, so whatever
    // comes up comes with an upload list inside the sweep list (both lists increase)
    const StreamList &sw = call->sweep;
    if (sw.listed) {
        static const std::string w5("kpilqr_iterate_streamed5");
        if (!kp_traj_list_ok(B, sw.count, sw.traj)) return set_err(c, KPILQR_ERR_ARG, w5 + ": sweep_traj must be strictly increasing and within [0, batch)");
        if (io->fd_slab) return set_err(c, KPILQR_ERR_ARG, w5 + ": io.fd_slab with sweep_traj (job lists carry their own trajectory indices: out of scope)");
        if (!u.listed && (call->kind != StreamPayload::none || io->r || io->r_x || io->r_u || io->u_nom || call->rx32 || call->ru32))
            return set_err(c, KPILQR_ERR_ARG, w5 + ": inputs with sweep_traj come with an upload_traj inside it");
        for (int i = 0, j = 0; i < u.count; i++) {
            while (j < sw.count && sw.traj[j] < u.traj[i]) j++;
            if (j == sw.count || sw.traj[j] != u.traj[i])
                return set_err(c, KPILQR_ERR_ARG, w5 + ": upload_traj lists trajectory " + std::to_string(u.traj[i]) + ", which sweep_traj does not (a re-linearised trajectory is an active one)");
        }
    }
    // (the refusals of kpilqr_upload_residuals_partial, in its words)
    const bool rx_given = io->r_x || call->rx32, ru_given = io->r_u || call->ru32;      // (either transport)
    if (u.listed && rx_given && c->rx_const_on)
        return set_err(c, KPILQR_ERR_STATE, w + ": the context holds constant residual Jacobians; a whole r_x through kpilqr_upload_residuals ends that mode first");
    if (u.listed && rx_given && !(c->rx_buf_valid && c->rx_whole))
        return set_err(c, KPILQR_ERR_STATE, w + ": r_x of a subset before a whole r_x: kpilqr_upload_residuals first");
    if (u.listed && ru_given && c->ru_zero)
        return set_err(c, KPILQR_ERR_STATE, w + ": r_u of a subset on a context that runs without control residuals: a whole r_u through kpilqr_upload_residuals first");
    const void *hostp[] = {kcols32, io->kp_columns, io->fd_kp_slab, io->fd_slab, io->r, io->r_x, io->r_u, io->u_nom, io->lambda, io->K, io->k, io->cost_pred, io->delta_J, io->status};
    for (const void *p : hostp) if (!is_pinned(p)) return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed: host buffers must be pinned (kpilqr_host_alloc)");
    if (call->K32) {
        if (io->K) return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed2: io.K and K32 are exclusive");
        if (!is_pinned(call->K32) || ((size_t)call->K32 & 7)) return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed2: K32 must be pinned (kpilqr_host_alloc) and 8-byte aligned");
    }
    // the Jacobians as FP32: per array one transport per call; the copy-kernel route reads the caller's floats in pairs
    if ((io->r_x && call->rx32) || (io->r_u && call->ru32))
        return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed6: io.r_x and r_x32 (io.r_u and r_u32) are exclusive: one transport per array and call");
    for (const float *p : {call->rx32, call->ru32})
        if (!is_pinned(p) || ((size_t)p & 7)) return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed6: r_x32 and r_u32 must be pinned (kpilqr_host_alloc) and 8-byte aligned");
    if (g.listed && !kp_traj_list_ok(B, g.count, g.traj))
        return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed2: gain_traj must be strictly increasing and within [0, batch)");
    if (c->fused) { const int rc = check_fused(c); if (rc) return rc; }
    if (!io->fd_slab) return KPILQR_OK;
    // the job lists' offsets, last: the one walk over the batch
    if (io->traj_job_first[0] != 0 || io->traj_job_first[B] != io->njobs)
        return set_err(c, KPILQR_ERR_ARG, "traj_job_first must run from 0 to njobs");
    unsigned long long h = 1469598103934665603ULL;
    auto mix = [&](unsigned long long v) { h = (h ^ v) * 1099511628211ULL; };
    mix((unsigned)io->njobs); mix((unsigned)io->nnom);
    for (int b = 0; b <= B; b++) {
        const int j = io->traj_job_first[b];
        if (j < 0 || j > io->njobs || (b > 0 && j < io->traj_job_first[b - 1]))
            return set_err(c, KPILQR_ERR_ARG, "traj_job_first not monotone in [0, njobs]");
        mix((unsigned)j);
        if (io->nnom > 0) {
            const int q = io->traj_nom_first[b];
            if (q < 0 || q > io->nnom || (b > 0 && q < io->traj_nom_first[b - 1]))
                return set_err(c, KPILQR_ERR_ARG, "traj_nom_first not monotone in [0, nnom]");
            mix((unsigned)q);
        }
    }
    *sig = h;
    return KPILQR_OK;
}

// The buffers the chunks upload into, sized on the context before a chunk is cut (a view never allocates), and what the context
// records about the payload that lands in them.  pay_entries: entries of the payload as it will be resident.
static int stream_reserve(kpilqr_ctx *c, StreamCall *call, unsigned long long sig, int pay_entries)
{
    const kpilqr_stream_io *io = call->io;
    const int n = c->n, B = c->d.batch;
    int rc;
    if (call->kind == StreamPayload::jobs) {
        // The device slab is laid out from (njobs, nnom) and a chunk's payload lands at its trajectories' job / nominal
        // ranges.  Same-stream order protects a chunk's ranges from the NEXT iteration's uploads only while those ranges
        // are the same; when the layout or the per-trajectory offsets differ from the iteration still in flight, the
        // new uploads could overwrite regions another chunk stream is still differencing -- so the pipeline is joined
        // first (every chunk stream then starts behind everything enqueued so far, through pipe_in below).
        kpilqr_fd_layout &L = call->L;
        fd_layout(n, io->njobs, io->nnom, &L);
        if (c->pipe_dirty && sig != c->pipe_sig) { rc = join_pipeline(c); if (rc) return rc; }
        rc = quiesce_for_growth(c, {{&c->fd_dev, L.bytes}}); if (rc) return rc;
        rc = fd_bind(c, io->njobs, io->nnom, &L);
        if (rc) return rc;
        c->pipe_sig = sig;
        c->njobs = io->njobs; c->nnom = io->nnom; c->eps = io->eps;
    }
    if (call->kind == StreamPayload::kp_ordered) {
        // a chunk's payload lands at its trajectories' entry range, which only the key-points decide: same-stream order
        // protects it from the next iteration's uploads (new key-points go through KP_ENTER, which joins the pipeline)
        kpilqr_fdkp_layout LK{};
        fdkp_layout(n, pay_entries, &LK);
        rc = quiesce_for_growth(c, {{&c->fdk_dev, LK.bytes}}); if (rc) return rc;      // as for the job-list slab
        rc = fdk_bind(c, pay_entries, &LK);
        if (rc) return rc;
        c->fdk_entries = pay_entries; c->fdk_first = 0; c->eps = io->eps;
    }
    if (call->kind == StreamPayload::columns_f32) {
        // The staging buffer the chunks upload into (shared with kpilqr_upload_kp_columns_f32[_partial], which join the pipeline on
        // entry): a chunk's floats land at its trajectories' entry range, which only the key-points decide, so same-stream order
        // protects it from the next iteration's upload as it does the key-point ordered slab.  A growth frees the old buffer, which nothing
        // may still read: as for the slabs
        rc = quiesce_for_growth(c, {{&c->kpc32, (size_t)pay_entries * call->rec}}); if (rc) return rc;
        rc = reserve_columns_f32(c, pay_entries);
        if (rc) return rc;
    }
    // Inputs of a list: the staging regions the chunks upload their compact slices into, one per input kind that is given, as large
    // as the whole-batch form of that input -- a chunk's slice lands where its first trajectory's rows (entries) would, which the
    // chunk alone decides, so same-stream order protects it from the next call's upload whatever that call lists.  Reserved here, on
    // the context, and kept; a growth frees the old region, which nothing may still read: as for the slabs.  (kp_columns32 stages
    // in kpc32, above.)
    const StreamList &u = call->rows;
    const bool stage_pay = u.listed && (call->kind == StreamPayload::kp_ordered || call->kind == StreamPayload::columns);
    if (u.listed && u.count > 0) {
        const RowSizes per = row_sizes(c);
        const size_t all = (size_t)B * sizeof(double);
        const size_t need[Ctx::kRowsKinds] = {io->r ? all * per.r : 0, io->r_x ? all * per.r_x : 0, io->r_u ? all * per.r_u : 0, io->u_nom ? all * per.u_nom : 0,
                                              stage_pay ? (size_t)pay_entries * call->rec : 0};
        DevBuf<char> *const stg = c->rows_stage;
        rc = quiesce_for_growth(c, {{&stg[0], need[0]}, {&stg[1], need[1]}, {&stg[2], need[2]}, {&stg[3], need[3]}, {&stg[4], need[4]}}); if (rc) return rc;
        for (int kd = 0; kd < Ctx::kRowsKinds; kd++) { rc = reserve(c, stg[kd], need[kd], kExact, false); if (rc < 0) return rc; }
        // the payload region is cut by entry * record size: records behind columns (or the other way round) would cut it elsewhere,
        // and a chunk's upload could land in a range another chunk stream is still reading -- the rule of pipe_sig
        if (stage_pay && c->rows_pay_rec != call->rec) { rc = join_pipeline(c); if (rc) return rc; c->rows_pay_rec = call->rec; }
    }
    // The Jacobians as FP32, uploads by SDMA: the staging buffer of kpilqr_upload_residual_jacobians_f32[_partial] (which join the
    // pipeline on entry), laid out [r_x32 | r_u32] at whole-batch size -- a chunk's slice lands where its first trajectory's rows
    // would, list or no list, so the chunk alone addresses a region and same-stream order protects it from the next call's upload, as
    // for rows_stage.  The copy-kernel route reads the caller's floats itself: nothing is reserved or touched.
    if ((call->rx32 || call->ru32) && !call->k_up && !(u.listed && u.count == 0)) {
        const RowSizes per = row_sizes(c);
        const size_t need = (size_t)B * (per.r_x + per.r_u) * sizeof(float);
        rc = quiesce_for_growth(c, {{&c->rj32, need}}); if (rc) return rc;
        rc = reserve(c, c->rj32, need, kExact, false); if (rc < 0) return rc;
    }
    if (call->kind == StreamPayload::jobs) c->fd_payload = FdPayload::jobs;
    if (call->kind == StreamPayload::kp_ordered) c->fd_payload = FdPayload::kp_ordered;
    if (call->kind == StreamPayload::columns || call->kind == StreamPayload::columns_f32) { c->fd_payload = FdPayload::kp_columns; c->fdk_entries = pay_entries; c->fdk_first = 0; }
    if (call->kind != StreamPayload::none) payload_changed(c);
    return KPILQR_OK;
}

// Phase 2 -- everything a streamed iteration does ONCE, on the context, before the chunks are cut.  Nothing here touches a chunk
// stream except through quiesce_for_growth and join_pipeline.
static int stream_prepare(kpilqr_ctx *c, StreamCall *call, unsigned long long sig)
{
    const kpilqr_stream_io *io = call->io;
    const int B = c->d.batch;
    int rc = pipe_setup(c);
    if (rc) return rc;
    if (call->nchunks < 1) call->nchunks = Ctx::kPipeStreams;          // 0: one chunk per pipeline stream
    if (call->nchunks > B) call->nchunks = B;
    // the chunk -> stream map must not change while earlier chunks are still in flight (same-stream order is what
    // protects a chunk's device buffers from the next iteration's uploads)
    if (c->pipe_dirty && c->pipe_chunks != call->nchunks) { rc = join_pipeline(c); if (rc) return rc; }
    c->pipe_chunks = call->nchunks;
    // uploads by SDMA, downloads by a copy kernel: the only pairing whose two directions overlap inside this pipeline
    // (KPILQR_PIPE_COPY: bit 0 uploads by kernel, bit 1 downloads by kernel; profiles/r02_pcie_inclusive.txt)
    const int pipe_copy = c->tune.pipe_copy >= 0 ? c->tune.pipe_copy : 2;
    call->k_up = pipe_copy & 1; call->k_down = pipe_copy & 2;
    // entries of the payload as it will be resident: with a list the kept trajectories' stay beside the ones that arrive
    rc = stream_reserve(c, call, sig, call->rows.listed ? c->kp_total_host : io->entries);
    if (rc) return rc;
    const bool new_payload = call->kind != StreamPayload::none, by_entry = call->by_entry();
    // allocations and tables the chunks need are made HERE, on the context: a view never allocates (reserve refuses)
    if (c->fused || payload_by_entry(c)) {
        rc = ensure_kpc(c); if (rc) return rc;
        rc = ensure_entry_tables(c); if (rc) return rc;
    }
    if (!c->fused && by_entry && c->tune.fd_interp != 0) { rc = ensure_segent(c); if (rc) return rc; }
    const StreamList &sw = call->sweep;
    // a listed chunk reads, or differences, its own entry range of a payload laid out by the lists: the host has to know them
    if (sw.listed && payload_by_entry(c) && !c->kp_traj_first_host) {
        rc = ensure_offsets_mirror(c); if (rc) return rc;
        if (!remember_traj_first(c, c->kp_offsets_host)) return set_err(c, KPILQR_ERR_ALLOC, "host allocation failed");
    }
    if (c->fused) {
        if (!sw.listed) c->last_linearise = "in_sweep";
        else if (sw.count > 0) c->last_linearise = "in_sweep:subset";
        // per-DoF lists: a chunk computes the slopes of ITS entries, whose range only the host copy of the lists gives
        if (!c->kp_known_uniform && !c->kp_traj_first_host)
            return set_err(c, KPILQR_ERR_STATE, "kpilqr_iterate_streamed with per-DoF key-point lists: the lists must be known to the host (kpilqr_set_keypoints, or kpilqr_get_keypoints after generating them)");
        rc = ensure_kps(c); if (rc) return rc;
    }
    // No new payload, but the column store of the resident one is stale (key-points changed since a job-list upload): a chunk
    // view has no jobs (its njobs is 0), so the payload is re-differenced HERE, on the context, for the whole batch -- what
    // kpilqr_iterate would do.  (A key-point ordered payload is dropped by new key-points; the chunks handle a resident one.)
    if (c->fused && !new_payload && !c->pay.kpc_valid && c->fd_payload == FdPayload::jobs) {
        rc = difference_to_kpc(c); if (rc) return rc;
    }
    // The same on a context with records: without a new payload a chunk runs k_interpolate alone, between the key-point columns its
    // records hold -- those of the resident payload only if something has written them there since it arrived.  A payload uploaded
    // by an ordinary call (kpilqr_upload_fd_kp, a partial upload behind kpilqr_update_keypoints ...) and not linearised yet is
    // written into the records HERE, for the whole batch, behind the chunks of any earlier iteration (rec_synced is cleared by
    // payload_changed, so this is the first sweep since that upload: the join costs an overlap nobody had).
    if (!c->fused && !new_payload && !c->pay.rec_synced && !sw.listed) {
        rc = join_pipeline(c); if (rc) return rc;
        rc = records_from_payload(c); if (rc) return rc;
    }
    // A sweep list on a context with records: the chunks linearise their listed trajectories as kpilqr_fd_interpolate_partial does,
    // from the resident payload, and nobody else's records are written.  Resident job lists are differenced HERE, once (a chunk view
    // has no jobs), whoever they belong to -- that call's rule -- behind the chunks of any earlier iteration.
    if (!c->fused && sw.listed && sw.count > 0 && c->fd_payload == FdPayload::jobs) {
        rc = join_pipeline(c); if (rc) return rc;
        KP_HIP(c, launch_fd_difference(c));
    }
    // Per-step Jacobians in this call end the constant mode -- recorded only HERE, behind every check that can still reject the
    // call (a rejected call must leave the context as it was: round-4 advisor; before, a call refused for an unpinned buffer had
    // already left the constant mode and the next sweep read an r_x buffer that never received the broadcast copy)
    if (io->r_u || call->ru32) c->ru_zero = false;
    if (io->r_x || call->rx32) { c->rx_const_on = false; c->rx_buf_valid = c->rx_whole = true; }
    // constant residual Jacobians and a kernel family that streams r_x: the broadcast copy is made here, on the context (the
    // chunks' wave organisation is the whole batch's: make_view gives a chunk its share of the SIMDs)
    if (!(c->fused && plan_backward_fused(c, false).rxc && plan_forward_fused(c).rxc)) { rc = ensure_rx_buffer(c); if (rc) return rc; }
    // the list of the gains that come down: on the device before the chunks, which read their slices of it
    rc = pipe_list_bind(c, call->gains); if (rc) return rc;
    // the list of the inputs that come up, in its ring slot (an empty list reads none)
    const StreamList &u = call->rows;
    if (u.listed && u.count > 0) {
        rc = rows_list_bind(c, u, call->nchunks, new_payload, &call->uslot); if (rc) return rc;
        call->ulist = (const int *)c->rows_list + (size_t)call->uslot * 2 * B; call->ufirst = call->ulist + B;
    }
    // the list of the trajectories that are swept, in a slot of its own ring (an empty list launches nothing that reads one)
    if (sw.listed && sw.count > 0) {
        rc = sweep_list_bind(c, sw, &call->sslot); if (rc) return rc;
        call->slist = (const int *)c->sweep_ring + (size_t)call->sslot * B;
    }
    // where a chunk's range of a by-entry payload lands, now that every buffer is there
    char *const stage = c->rows_stage[Ctx::kRowsPayload];
    if (call->kind == StreamPayload::kp_ordered) { call->place = c->fdk_dev.p; call->land = u.listed ? stage : (char *)c->fdk_dev.p; }
    if (call->kind == StreamPayload::columns) { call->place = c->kpc.p; call->land = u.listed ? stage : (char *)c->kpc.p; }
    if (call->kind == StreamPayload::columns_f32) call->land = (char *)c->kpc32.p;
    // order the chunk streams behind whatever the caller enqueued on the context's stream so far (key-points, weights ...)
    KP_HIP(c, hipEventRecord(c->pipe_in, c->stream));
    // from here on chunk streams hold work: every exit path, errors included, leaves the pipeline marked for joining, so a
    // later kpilqr_sync / kpilqr_destroy waits for the DMAs that read the caller's buffers
    c->pipe_dirty = true;
    return KPILQR_OK;
}

// One chunk of a streamed iteration: trajectories [b0, b1) as the view v on stream s, and its slices of the upload and sweep lists
struct StreamChunk {
    int ch = 0, b0 = 0, b1 = 0;
    hipStream_t s = nullptr;
    kpilqr_ctx v;
    int u0 = 0, urows = 0;             // inputs of a list: rows [u0, u0 + urows) of every compact input ...
    size_t uent0 = 0, uents = 0;       // ... and, of a by-entry payload, `uents` entries from entry uent0 on
    int s0 = 0, srows = 0;             // sweeps of a list: entries [s0, s0 + srows) of the sweep list, and of every compact small array
};

// The chunk's FD payload: uploaded, and the view told what it holds
static int stream_chunk_payload(kpilqr_ctx *c, const StreamCall &call, StreamChunk &k)
{
    const kpilqr_stream_io *io = call.io;
    kpilqr_ctx &v = k.v;
    hipStream_t s = k.s;
    const int n = c->n;
    if (call.kind == StreamPayload::jobs) {
        const kpilqr_fd_layout &L = call.L;
        const char *slab = (const char *)io->fd_slab;
        const int j0 = io->traj_job_first[k.b0], j1 = io->traj_job_first[k.b1];
        const size_t J = (size_t)(j1 - j0), jo = (size_t)j0;
        if (J) {
            KP_HIP(c, call.h2d(c->xplus + jo * n, slab + L.xplus + jo * n * 8, J * n * 8, s));
            KP_HIP(c, call.h2d(c->xminus + jo * n, slab + L.xminus + jo * n * 8, J * n * 8, s));
            KP_HIP(c, call.h2d(c->job_b + jo, slab + L.job_b + jo * 4, J * 4, s));
            KP_HIP(c, call.h2d(c->job_t + jo, slab + L.job_t + jo * 4, J * 4, s));
            KP_HIP(c, call.h2d(c->job_col + jo, slab + L.job_col + jo * 4, J * 4, s));
            KP_HIP(c, call.h2d(c->job_nom + jo, slab + L.job_nom + jo * 4, J * 4, s));
            KP_HIP(c, call.h2d(c->job_mode + jo, slab + L.job_mode + jo, J, s));
        }
        if (io->nnom > 0) {
            const int q0 = io->traj_nom_first[k.b0], q1 = io->traj_nom_first[k.b1];
            if (q1 > q0) KP_HIP(c, call.h2d(c->xnom + (size_t)q0 * n, slab + L.xnom + (size_t)q0 * n * 8, (size_t)(q1 - q0) * n * 8, s));
        }
        // the chunk's jobs: a contiguous range of the job arrays
        v.job_b = c->job_b + jo; v.job_t = c->job_t + jo; v.job_col = c->job_col + jo; v.job_nom = c->job_nom + jo;
        v.job_mode = c->job_mode + jo; v.xplus = c->xplus + jo * n; v.xminus = c->xminus + jo * n; v.njobs = (int)J;
    } else if (call.by_entry()) {
        // ONE copy of ONE contiguous range to where the chunk's first entry sits in `land`: the chunk's own entries (the view's range)
        // straight into place, or with a list its compact slice into the staging region; then at most ONE launch: FP32 columns are
        // widened into the column store (columns_f32.hip; the context's absolute tables; with a list, of the listed trajectories
        // alone), FP64 payloads of a list moved to the listed trajectories' entry ranges.  The view is the whole chunk's either way.
        const bool listed = call.rows.listed;
        const size_t rec = call.rec, e0 = (size_t)v.fdk_first, first = listed ? k.uent0 : e0, count = listed ? k.uents : (size_t)v.kp_view_entries;
        if (count) {
            KP_HIP(c, call.h2d(call.land + e0 * rec, call.src + first * rec, count * rec, s));
            if (call.kind == StreamPayload::columns_f32) KP_HIP(c, launch_kp_columns_f32_range(c, s, k.b0 * c->d.dof, k.b1 * c->d.dof, c->kpc32, call.ufirst));
            else if (listed) KP_HIP(c, launch_rows_in_entries(c, s, call.ulist + k.u0, k.urows, call.ufirst, rec, call.land, call.place));
        }
        v.njobs = 0; v.fdk_entries = v.kp_view_entries;      // the chunk's entries
        if (call.kind != StreamPayload::kp_ordered) v.pay.kpc_valid = true;
    } else {
        // no new FD payload: what was differenced before is reused (kpc / the records' key-point columns)
        v.njobs = 0;
        if (payload_by_entry(c) && c->kp_traj_first_host) v.fdk_entries = v.kp_view_entries;
    }
    return KPILQR_OK;
}

// The chunk's rows of r, r_x, r_u, u_nom (those that are given) and its lambdas
static int stream_chunk_rows(kpilqr_ctx *c, const StreamCall &call, StreamChunk &k)
{
    const kpilqr_stream_io *io = call.io;
    const RowSizes sz = row_sizes(c);
    const size_t o = k.b0, cnt = k.b1 - k.b0;
    const double *const src[Ctx::kRowsPayload] = {io->r, io->r_x, io->r_u, io->u_nom};
    double *const dst[Ctx::kRowsPayload] = {c->r, c->r_x, c->r_u, c->u_nom};
    const size_t pers[Ctx::kRowsPayload] = {sz.r, sz.r_x, sz.r_u, sz.u_nom};
    for (int kd = 0; kd < Ctx::kRowsPayload; kd++) {
        const size_t per = pers[kd];
        if (!src[kd]) continue;
        if (!call.rows.listed) {
            KP_HIP(c, call.h2d(dst[kd] + o * per, src[kd] + o * per, cnt * per * 8, k.s));
        } else if (k.urows) {
            // of a list: ONE upload of the chunk's rows into its staging region (at the chunk's first trajectory), ONE launch of
            // k_rows_in (rows_in.hip) to the listed trajectories' places in the CONTEXT's buffer
            double *const stg = (double *)c->rows_stage[kd].p + o * per;
            KP_HIP(c, call.h2d(stg, src[kd] + (size_t)k.u0 * per, (size_t)k.urows * per * 8, k.s));
            KP_HIP(c, launch_rows_in(k.s, call.ulist + k.u0, k.urows, (long long)per, stg, dst[kd]));
        }
    }
    // r_x / r_u as FP32: the chunk's rows -- its own, or its slice of the compact listed ones -- widened into the CONTEXT's buffers by
    // ONE launch for both arrays (residuals_f32.hip), from the chunk's region of the staging buffer behind ONE upload per array, or
    // (uploads by kernel) from the caller's pinned floats themselves
    const size_t frows = call.rows.listed ? (size_t)k.urows : cnt;
    if ((call.rx32 || call.ru32) && frows) {
        const size_t first = call.rows.listed ? (size_t)k.u0 : o;
        const float *fx = call.rx32 ? call.rx32 + first * sz.r_x : nullptr, *fu = call.ru32 ? call.ru32 + first * sz.r_u : nullptr;
        if (!call.k_up) {
            float *const stx = (float *)c->rj32 + o * sz.r_x, *const stu = (float *)c->rj32 + (size_t)c->d.batch * sz.r_x + o * sz.r_u;
            if (fx) { KP_HIP(c, call.h2d(stx, fx, frows * sz.r_x * sizeof(float), k.s)); fx = stx; }
            if (fu) { KP_HIP(c, call.h2d(stu, fu, frows * sz.r_u * sizeof(float), k.s)); fu = stu; }
        }
        KP_HIP(c, launch_widen_jacobians(k.s, call.rows.listed ? call.ulist + k.u0 : nullptr, k.b0, (int)frows, (long long)sz.r_x, fx, c->r_x,
                                         (long long)sz.r_u, fu, c->r_u));
    }
    // (the slot of the list may be written again once this stream has passed here)
    if (k.urows) {
        KP_HIP(c, hipEventRecord(c->rows_read[call.uslot][k.ch % Ctx::kPipeStreams], k.s));
        c->rows_read_set[call.uslot][k.ch % Ctx::kPipeStreams] = true;
    }
    // the lambdas: the chunk's own, or with a sweep list its slice of the compact ones, placed by ONE launch of k_rows_in that reads the
    // caller's pinned rows itself (a few doubles: no staging region, no ring)
    if (io->lambda && !call.sweep.listed) KP_HIP(c, call.h2d(k.v.lambda, io->lambda + o, cnt * 8, k.s));
    if (io->lambda && call.sweep.listed) KP_HIP(c, launch_rows_in(k.s, call.slist + k.s0, k.srows, 1, io->lambda + k.s0, c->lambda));
    return KPILQR_OK;
}

// A chunk's list view: make_view and make_list_view combined.  The context's unshifted per-trajectory pointers and whole payload,
// block i of a launch finds its trajectory through `list` -- the chunk's slice of the device copy of the sweep list, `count` long:
// the launch width -- on the chunk's stream and the chunk's share of the SIMDs; what the chunk did to the payload-derived state so far.
static void make_chunk_list_view(const kpilqr_ctx *c, const kpilqr_ctx &chunk, const int *list, int count, kpilqr_ctx *v)
{
    *v = *c;
    v->is_view = true;
    v->own_stream = false;
    v->stream = chunk.stream;
    v->n_simd = chunk.n_simd;
    v->pay = chunk.pay;
    v->d.batch = count;
    v->sweep_list = list;
}

// The chunk's kernels with a sweep list: what kpilqr_iterate_partial launches for the chunk's slice of the list, on the chunk's stream
static int stream_chunk_sweeps_listed(kpilqr_ctx *c, const StreamCall &call, StreamChunk &k)
{
    const kpilqr_stream_io *io = call.io;
    kpilqr_ctx &v = k.v;
    const auto of = [&](const kpilqr_ctx &w, int rcv) { if (rcv) c->err = w.err; return rcv; };      // a view's refusal is the context's
    int rc;
    // The chunk's entry range of the column store, where the listed launches read it: a listed sweep never differences inside the
    // sweep (columns_for_listed_sweep), and under KPILQR_FD_INTERP=0 the records' key-point steps are written from it.  A range
    // that is not valid is differenced here, whoever is listed: every chunk leaves its range valid, so the store is for the context.
    const bool one_pass = !c->fused && linearise_one_pass(&v);
    if (c->fused) rc = of(v, columns_for_listed_sweep(&v));
    else rc = (!one_pass && payload_by_entry(&v) && !v.pay.kpc_valid) ? of(v, difference_to_kpc(&v)) : KPILQR_OK;
    if (rc) return rc;
    if (!k.srows) return KPILQR_OK;
    const int *const list = call.slist + k.s0;
    kpilqr_ctx lv;
    make_chunk_list_view(c, v, list, k.srows, &lv);
    if (!c->fused) {
        // kpilqr_fd_interpolate_partial's launches, then kpilqr_cost_derivs_partial's
        if (one_pass) {
            KP_HIP(c, launch_fd_kp_interpolate(&lv, list, k.srows));
            c->last_linearise = c->fd_payload == FdPayload::kp_columns ? "kp_columns_interpolate:subset" : "fd_kp_interpolate:subset";
        } else {
            if (payload_by_entry(c)) { rc = of(lv, kpc_to_records_of(&lv, k.srows, call.sweep.traj + k.s0)); if (rc) return rc; }
            KP_HIP(c, launch_interpolate(&lv, list, k.srows));
            c->last_linearise = "fd_difference+interpolate:subset";
        }
        if (!c->tiled_a6) KP_HIP(c, launch_cost_derivs(&lv, list, k.srows));
    }
    c->retry_attempts = retry_attempts_for(c, io->lambda ? io->lambda + k.s0 : nullptr, (size_t)k.srows);      // (the slice's own lambdas decide its attempts)
    rc = launch_backward_listed(c, &lv, call.pd_check_stride);
    if (rc) return rc;
    return launch_forward_listed(c, &lv, nullptr);
}

// The chunk's kernels: the ordinary launchers on the view
static int stream_chunk_sweeps(kpilqr_ctx *c, const StreamCall &call, StreamChunk &k)
{
    if (call.sweep.listed) return stream_chunk_sweeps_listed(c, call, k);
    const kpilqr_stream_io *io = call.io;
    kpilqr_ctx &v = k.v;
    const size_t o = k.b0, cnt = k.b1 - k.b0;
    const auto of_view = [&](int rcv) { if (rcv) c->err = v.err; return rcv; };      // a view's refusal is the context's
    int rc;
    if (!c->fused) {
        // (no new payload: the records hold its key-point columns already)
        rc = of_view(linearise(&v, call.kind != StreamPayload::none));
        if (rc) return rc;
        c->last_linearise = v.last_linearise;
        if (!c->tiled_a6) KP_HIP(c, launch_cost_derivs(&v));
    }
    v.retry_attempts = retry_attempts_for(c, io->lambda ? io->lambda + o : nullptr, cnt);      // (the chunk's own lambdas decide its attempts)
    rc = of_view(run_backward(&v, call.pd_check_stride));
    if (rc) return rc;
    c->retry_ran = v.retry_ran;
    rc = of_view(run_forward(&v, nullptr));
    if (rc) return rc;
    c->last_bwd = v.last_bwd; c->last_fwd = v.last_fwd;
    c->last_width[0] = c->last_width[1] = -1;      // (whole chunks: not a listed launch, whatever ran before)
    return KPILQR_OK;
}

// The chunk's outputs.  K, k by a copy kernel: it overlaps with the SDMA uploads of the next chunks (two SDMA directions do not)
static int stream_chunk_down(kpilqr_ctx *c, StreamCall &call, StreamChunk &k)
{
    const kpilqr_stream_io *io = call.io;
    const kpilqr_ctx &v = k.v;
    hipStream_t s = k.s;
    StreamList &g = call.gains;
    const RowSizes per = row_sizes(c);
    const size_t na = c->d.n_alpha, o = k.b0, cnt = k.b1 - k.b0;
    const bool gather = call.K32 || g.listed;      // K (and k of a list) leave through gains.hip's gather kernel
    if (gather) {
        // K32 and the rows of a list: gathered (and rounded) by ONE launch per array straight into the pinned destination, whatever
        // KPILQR_PIPE_COPY says (through SDMA they would need a staging buffer).  The chunk's share of a list is one slice of it,
        // [i0, i1), and one contiguous range of the compact outputs; without a list it is the chunk's own rows.
        int i0 = k.b0, i1 = k.b1;
        if (g.listed) g.slice_below(k.b1, &i0, &i1);
        const int *tl = g.listed ? (const int *)c->pipe_list + i0 : nullptr;
        if (call.K32) KP_HIP(c, launch_gains_out(c, s, GainsForm::K_f32, tl, k.b0, i1 - i0, call.K32 + (size_t)i0 * per.K));
        else if (io->K) KP_HIP(c, launch_gains_out(c, s, GainsForm::K_f64, tl, k.b0, i1 - i0, io->K + (size_t)i0 * per.K));
        if (io->k && g.listed) KP_HIP(c, launch_gains_out(c, s, GainsForm::k_f64, tl, k.b0, i1 - i0, io->k + (size_t)i0 * per.k));
    }
    // K and k of the whole batch (k: the copy it always was, beside K32 too), by the copy kernel unless KPILQR_PIPE_COPY says SDMA
    const auto d2h = [&](double *dst, const double *src, size_t count) {
        return call.k_down ? launch_copy_out(s, dst, src, count) : hipMemcpyAsync(dst, src, count * 8, hipMemcpyDeviceToHost, s);
    };
    if (io->K && !gather) KP_HIP(c, d2h(io->K + o * per.K, v.K, cnt * per.K));
    if (io->k && !g.listed) KP_HIP(c, d2h(io->k + o * per.k, v.k, cnt * per.k));
    if (call.sweep.listed) {
        // the small outputs of a sweep list: the chunk's slice of the compact arrays, gathered by ONE launch per array straight into
        // the caller's pinned rows (the route of k_gains_out: no staging buffer, no second DMA)
        if (!k.srows) return KPILQR_OK;
        const int *const list = call.slist + k.s0;
        const size_t i0 = (size_t)k.s0;
        if (io->cost_pred) KP_HIP(c, launch_rows_out(s, list, k.srows, 2 * (int)na, (const double *)c->cost_pred, io->cost_pred + i0 * na));
        if (io->delta_J) KP_HIP(c, launch_rows_out(s, list, k.srows, 2, (const double *)c->delta_J, io->delta_J + i0));
        if (io->status) KP_HIP(c, launch_rows_out(s, list, k.srows, 1, (const int *)c->status, io->status + i0));
        // (the slot of the sweep list may be written again once this stream has passed here)
        KP_HIP(c, hipEventRecord(c->sweep_read[call.sslot][k.ch % Ctx::kPipeStreams], s));
        c->sweep_read_set[call.sslot][k.ch % Ctx::kPipeStreams] = true;
        return KPILQR_OK;
    }
    if (io->cost_pred) KP_HIP(c, hipMemcpyAsync(io->cost_pred + o * na, v.cost_pred, cnt * na * 8, hipMemcpyDeviceToHost, s));
    if (io->delta_J) KP_HIP(c, hipMemcpyAsync(io->delta_J + o, v.delta_J, cnt * 8, hipMemcpyDeviceToHost, s));
    if (io->status) KP_HIP(c, hipMemcpyAsync(io->status + o, v.status, cnt * 4, hipMemcpyDeviceToHost, s));
    return KPILQR_OK;
}

// A streamed iteration in three phases: every refusal (stream_check), everything done once on the context (stream_prepare), then
// per chunk the payload, the rows, the sweeps and the downloads, each chunk on its own stream.
static int iterate_streamed(kpilqr_ctx *c, StreamCall call)
{
    KP_HIP(c, hipSetDevice(c->d.device));
    unsigned long long sig = 0;
    int rc = stream_check(c, &call, &sig);
    if (rc) return rc;
    rc = stream_prepare(c, &call, sig);
    if (rc) return rc;
    // What the chunks do to the payload-derived state comes back from the LAST view, whole (every chunk does the same to its slice
    // of kpc, kps and the records; a view never takes the union route, so kpcu_valid returns as it left).  Nothing of ListsDerived
    // comes back: a view builds no table -- the context ensured them above.
    PayloadDerived after = c->pay;
    const int B = c->d.batch;
    StreamList &u = call.rows;
    StreamChunk k;
    size_t uent = 0;                            // payload entries of the listed trajectories below the chunk
    for (k.ch = 0; k.ch < call.nchunks; k.ch++) {
        k.b0 = chunk_first(B, k.ch, call.nchunks); k.b1 = chunk_first(B, k.ch + 1, call.nchunks);
        if (k.b1 <= k.b0) continue;
        k.s = c->pipe_stream[k.ch % Ctx::kPipeStreams];
        KP_HIP(c, hipStreamWaitEvent(k.s, c->pipe_in, 0));
        make_view(c, k.b0, k.b1 - k.b0, k.s, &k.v);
        // inputs of a list: the chunk's share is one slice of the list, and of a by-entry payload the entries of that slice
        int u1 = 0;
        if (u.listed) u.slice_below(k.b1, &k.u0, &u1);
        k.urows = u1 - k.u0; k.uent0 = uent;
        if (call.by_entry())
            for (int i = k.u0; i < u1; i++) uent += (size_t)(c->kp_traj_first_host[u.traj[i] + 1] - c->kp_traj_first_host[u.traj[i]]);
        k.uents = uent - k.uent0;
        int s1 = 0;
        if (call.sweep.listed) call.sweep.slice_below(k.b1, &k.s0, &s1);
        k.srows = s1 - k.s0;
        rc = stream_chunk_payload(c, call, k); if (rc) return rc;
        rc = stream_chunk_rows(c, call, k); if (rc) return rc;
        rc = stream_chunk_sweeps(c, call, k); if (rc) return rc;
        after = k.v.pay;
        rc = stream_chunk_down(c, call, k); if (rc) return rc;
    }
    c->pay = after;
    return KPILQR_OK;
}

int kpilqr_iterate_streamed(kpilqr_ctx *c, const kpilqr_stream_io *io, int pd_check_stride, int nchunks)
{
    KP_NOT_EMBEDDED(c, "kpilqr_iterate_streamed");
    if (!c || !io) return KPILQR_ERR_ARG;
    return iterate_streamed(c, StreamCall(io, pd_check_stride, nchunks));
}

// the checks and the options of a kpilqr_stream_io2, for the three calls that carry one
static int stream_gains_of(kpilqr_ctx *c, const kpilqr_stream_io2 *io2, StreamCall *call)
{
    if (io2->struct_size != sizeof(kpilqr_stream_io2)) return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed2: struct_size is not sizeof(kpilqr_stream_io2) of this library");
    if (io2->gain_count < 0 || (io2->gain_count > 0 && !io2->gain_traj)) return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed2: gain_count < 0, or listed trajectories without gain_traj");
    call->K32 = io2->K32;
    call->gains.listed = io2->gain_traj != nullptr; call->gains.count = io2->gain_count; call->gains.traj = io2->gain_traj;
    return KPILQR_OK;
}

int kpilqr_iterate_streamed2(kpilqr_ctx *c, const kpilqr_stream_io2 *io2, int pd_check_stride, int nchunks)
{
    KP_NOT_EMBEDDED(c, "kpilqr_iterate_streamed2");
    if (!c || !io2) return KPILQR_ERR_ARG;
    StreamCall call(&io2->io, pd_check_stride, nchunks);
    if (const int rc = stream_gains_of(c, io2, &call)) return rc;
    return iterate_streamed(c, call);
}

// kpilqr_iterate_streamed2 with the key-point columns as ENCODED FP32 for a payload: with kp_columns32 == NULL it IS that call
int kpilqr_iterate_streamed3(kpilqr_ctx *c, const kpilqr_stream_io3 *io3, int pd_check_stride, int nchunks)
{
    KP_NOT_EMBEDDED(c, "kpilqr_iterate_streamed3");
    if (!c || !io3) return KPILQR_ERR_ARG;
    if (io3->struct_size != sizeof(kpilqr_stream_io3)) return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed3: struct_size is not sizeof(kpilqr_stream_io3) of this library");
    StreamCall call(&io3->io2.io, pd_check_stride, nchunks);
    if (const int rc = stream_gains_of(c, &io3->io2, &call)) return rc;
    call.kcols32 = io3->kp_columns32;
    return iterate_streamed(c, call);
}

// kpilqr_iterate_streamed3 taking the inputs of a list of trajectories alone: with upload_traj == NULL it IS that call
// the checks and the options of a kpilqr_stream_io4, for the two calls that carry one (call->io is &io4->io3.io2.io)
static int stream_rows_of(kpilqr_ctx *c, const kpilqr_stream_io4 *io4, StreamCall *call)
{
    if (io4->struct_size != sizeof(kpilqr_stream_io4)) return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed4: struct_size is not sizeof(kpilqr_stream_io4) of this library");
    const kpilqr_stream_io3 *io3 = &io4->io3;
    if (io3->struct_size != sizeof(kpilqr_stream_io3)) return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed3: struct_size is not sizeof(kpilqr_stream_io3) of this library");
    if (io4->upload_count < 0 || (io4->upload_count > 0 && !io4->upload_traj))
        return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed4: upload_count < 0, or listed trajectories without upload_traj");
    if (const int rc = stream_gains_of(c, &io3->io2, call)) return rc;
    call->kcols32 = io3->kp_columns32;
    call->rows.listed = io4->upload_traj != nullptr; call->rows.count = call->rows.listed ? io4->upload_count : 0; call->rows.traj = io4->upload_traj;
    return KPILQR_OK;
}

int kpilqr_iterate_streamed4(kpilqr_ctx *c, const kpilqr_stream_io4 *io4, int pd_check_stride, int nchunks)
{
    KP_NOT_EMBEDDED(c, "kpilqr_iterate_streamed4");
    if (!c || !io4) return KPILQR_ERR_ARG;
    StreamCall call(&io4->io3.io2.io, pd_check_stride, nchunks);
    if (const int rc = stream_rows_of(c, io4, &call)) return rc;
    return iterate_streamed(c, call);
}

// kpilqr_iterate_streamed4 linearising and sweeping a list of trajectories alone: with sweep_traj == NULL it IS that call
// the checks and the options of a kpilqr_stream_io5, for the two calls that carry one (call->io is &io5->io4.io3.io2.io)
static int stream_sweep_of(kpilqr_ctx *c, const kpilqr_stream_io5 *io5, StreamCall *call)
{
    if (io5->struct_size != sizeof(kpilqr_stream_io5)) return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed5: struct_size is not sizeof(kpilqr_stream_io5) of this library");
    if (const int rc = stream_rows_of(c, &io5->io4, call)) return rc;
    if (io5->sweep_count < 0 || (io5->sweep_count > 0 && !io5->sweep_traj))
        return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed5: sweep_count < 0, or listed trajectories without sweep_traj");
    call->sweep.listed = io5->sweep_traj != nullptr; call->sweep.count = call->sweep.listed ? io5->sweep_count : 0; call->sweep.traj = io5->sweep_traj;
    return KPILQR_OK;
}

int kpilqr_iterate_streamed5(kpilqr_ctx *c, const kpilqr_stream_io5 *io5, int pd_check_stride, int nchunks)
{
    KP_NOT_EMBEDDED(c, "kpilqr_iterate_streamed5");
    if (!c || !io5) return KPILQR_ERR_ARG;
    StreamCall call(&io5->io4.io3.io2.io, pd_check_stride, nchunks);
    if (const int rc = stream_sweep_of(c, io5, &call)) return rc;
    return iterate_streamed(c, call);
}

// kpilqr_iterate_streamed5 taking the per-step residual Jacobians as FP32 inside the chunks: with r_x32 == r_u32 == NULL it IS that call
int kpilqr_iterate_streamed6(kpilqr_ctx *c, const kpilqr_stream_io6 *io6, int pd_check_stride, int nchunks)
{
    KP_NOT_EMBEDDED(c, "kpilqr_iterate_streamed6");
    if (!c || !io6) return KPILQR_ERR_ARG;
    if (io6->struct_size != sizeof(kpilqr_stream_io6)) return set_err(c, KPILQR_ERR_ARG, "kpilqr_iterate_streamed6: struct_size is not sizeof(kpilqr_stream_io6) of this library");
    StreamCall call(&io6->io5.io4.io3.io2.io, pd_check_stride, nchunks);
    if (const int rc = stream_sweep_of(c, &io6->io5, &call)) return rc;
    call.rx32 = io6->r_x32; call.ru32 = io6->r_u32;
    return iterate_streamed(c, call);
}

// ---- multi-GPU: the line-search cost reduction -----------------------------------------------------------
int kpilqr_comm_unique_id(char id[128])
{
    if (!id) return KPILQR_ERR_ARG;
    if (const char *e = comm_unique_id(id)) return set_err(nullptr, KPILQR_ERR_HIP, std::string("RCCL: ") + e);
    return KPILQR_OK;
}

int kpilqr_comm_init(kpilqr_ctx *c, int nranks, int rank, const char id[128])
{
    if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return KPILQR_ERR_ARG;
    if (c->comm) return set_err(c, KPILQR_ERR_STATE, "communicator already initialised");
    KP_HIP(c, hipSetDevice(c->d.device));
    if (const char *e = comm_init(c, nranks, rank, id)) return set_err(c, KPILQR_ERR_HIP, std::string("RCCL: ") + e);
    return KPILQR_OK;
}

int kpilqr_allreduce_linesearch(kpilqr_ctx *c, double vec8[8])
{
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    { const int rcg = reserve(c, c->ls8, 8 * sizeof(double), kExact, false); if (rcg < 0) return rcg; }
    KP_HIP(c, launch_pack_linesearch(c, c->ls8));
    if (const char *e = comm_allreduce8(c, c->ls8)) return set_err(c, KPILQR_ERR_HIP, std::string("RCCL: ") + e);
    if (vec8) KP_HIP(c, hipMemcpyAsync(vec8, c->ls8, 8 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return KPILQR_OK;
}

// ---- debug / oracle hooks -------------------------------------------------------------------------
// Staging of the reference layout, shared by each set / get pair: the records exist (a fused context materialises them), and the
// staging area holds the arrays one behind the other -- A | B, or l_x | l_xx | l_u | l_uu
struct Staged { size_t bytes[4]; double *dev[4]; };

static int stage_arrays(kpilqr_ctx *c, int count, Staged *s)
{
    if (c->fused) { const int rc = ensure_records(c); if (rc) return rc; }
    size_t total = 0;
    for (int i = 0; i < count; i++) total += s->bytes[i];
    const int rc = ensure_stage(c, total);
    if (rc) return rc;
    size_t off = 0;
    for (int i = 0; i < count; i++) { s->dev[i] = c->stage + off / 8; off += s->bytes[i]; }
    return KPILQR_OK;
}

static int stage_AB(kpilqr_ctx *c, Staged *s)
{
    const size_t BT = (size_t)c->d.batch * c->d.T, n = c->n, m = c->d.m;
    *s = Staged{{BT * n * n * 8, BT * n * m * 8}, {}};
    return stage_arrays(c, 2, s);
}

static int stage_cost(kpilqr_ctx *c, Staged *s)
{
    const size_t BT = (size_t)c->d.batch * c->d.T, n = c->n, m = c->d.m;
    *s = Staged{{BT * n * 8, BT * n * n * 8, BT * m * 8, BT * m * m * 8}, {}};
    return stage_arrays(c, 4, s);
}

int kpilqr_set_AB(kpilqr_ctx *c, const double *A, const double *B)
{
    KP_NOT_EMBEDDED(c, "kpilqr_set_AB");
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    Staged s;
    const int rc = stage_AB(c, &s);
    if (rc) return rc;
    const double *src[2] = {A, B};
    for (int i = 0; i < 2; i++)
        if (src[i]) KP_HIP(c, hipMemcpyAsync(s.dev[i], src[i], s.bytes[i], hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, launch_pack_AB(c, A ? s.dev[0] : nullptr, B ? s.dev[1] : nullptr));
    KP_HIP(c, hipStreamSynchronize(c->stream));
    return KPILQR_OK;
}

int kpilqr_get_AB(kpilqr_ctx *c, double *A, double *B)
{
    KP_NOT_EMBEDDED(c, "kpilqr_get_AB");
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    { const int rcp = check_complete(c, "kpilqr_get_AB"); if (rcp) return rcp; }
    Staged s;
    const int rc = stage_AB(c, &s);
    if (rc) return rc;
    KP_HIP(c, launch_unpack_AB(c, A ? s.dev[0] : nullptr, B ? s.dev[1] : nullptr));
    double *dst[2] = {A, B};
    for (int i = 0; i < 2; i++)
        if (dst[i]) KP_HIP(c, hipMemcpyAsync(dst[i], s.dev[i], s.bytes[i], hipMemcpyDeviceToHost, c->stream));
    return sync_and_report(c);
}

int kpilqr_set_cost_derivs(kpilqr_ctx *c, const double *l_x, const double *l_xx, const double *l_u, const double *l_uu)
{
    KP_NOT_EMBEDDED(c, "kpilqr_set_cost_derivs");
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    Staged s;
    const int rc = stage_cost(c, &s);
    if (rc) return rc;
    const double *src[4] = {l_x, l_xx, l_u, l_uu};
    for (int i = 0; i < 4; i++)
        if (src[i]) KP_HIP(c, hipMemcpyAsync(s.dev[i], src[i], s.bytes[i], hipMemcpyHostToDevice, c->stream));
    KP_HIP(c, launch_pack_cost(c, l_x ? s.dev[0] : nullptr, l_xx ? s.dev[1] : nullptr, l_u ? s.dev[2] : nullptr, l_uu ? s.dev[3] : nullptr));
    KP_HIP(c, hipStreamSynchronize(c->stream));
    return KPILQR_OK;
}

int kpilqr_get_cost_derivs(kpilqr_ctx *c, double *l_x, double *l_xx, double *l_u, double *l_uu)
{
    KP_NOT_EMBEDDED(c, "kpilqr_get_cost_derivs");
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    Staged s;
    const int rc = stage_cost(c, &s);
    if (rc) return rc;
    KP_HIP(c, launch_unpack_cost(c, l_x ? s.dev[0] : nullptr, l_xx ? s.dev[1] : nullptr, l_u ? s.dev[2] : nullptr, l_uu ? s.dev[3] : nullptr));
    double *dst[4] = {l_x, l_xx, l_u, l_uu};
    for (int i = 0; i < 4; i++)
        if (dst[i]) KP_HIP(c, hipMemcpyAsync(dst[i], s.dev[i], s.bytes[i], hipMemcpyDeviceToHost, c->stream));
    return sync_and_report(c);
}

// ---- the union of KPILQR_FLAG_UNION_KEYPOINTS, read back (both build it on demand; synchronous) ----------------------------------
int kpilqr_get_union_keypoints(kpilqr_ctx *c, int *traj_offsets, int *times, int times_capacity)
{
    KP_NOT_EMBEDDED(c, "kpilqr_get_union_keypoints");
    if (!c || !traj_offsets) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (!c->union_on) return set_err(c, KPILQR_ERR_STATE, "kpilqr_get_union_keypoints: KPILQR_FLAG_UNION_KEYPOINTS is not active on this context");
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "no key-points set");
    const int rc = ensure_union(c);
    if (rc) return rc;
    const int B = c->d.batch, dof = c->d.dof, total = c->kpu_total;
    memcpy(traj_offsets, c->kpu_traj_first_host, sizeof(int) * ((size_t)B + 1));
    if (times) {
        if (total > times_capacity) return set_err(c, KPILQR_ERR_ARG, "union times capacity too small");
        // every DoF list of a trajectory holds the same times: the first one is copied out
        for (int b = 0; b < B; b++) {
            const int f0 = traj_offsets[b], cnt = traj_offsets[b + 1] - f0;
            KP_HIP(c, hipMemcpyAsync(times + f0, c->kpu_times + (size_t)dof * f0, sizeof(int) * (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
        }
    }
    { const int rcs = sync_and_report(c); if (rcs) return rcs; }
    return total;
}

int kpilqr_get_union_columns(kpilqr_ctx *c, double *columns, size_t capacity_doubles)
{
    KP_NOT_EMBEDDED(c, "kpilqr_get_union_columns");
    if (!c) return KPILQR_ERR_ARG;
    KP_ENTER(c);
    if (!c->union_on) return set_err(c, KPILQR_ERR_STATE, "kpilqr_get_union_columns: KPILQR_FLAG_UNION_KEYPOINTS is not active on this context");
    if (!c->have_kp) return set_err(c, KPILQR_ERR_STATE, "no key-points set");
    if (c->fd_payload == FdPayload::none) return set_err(c, KPILQR_ERR_STATE, "kpilqr_get_union_columns: no FD payload resident");
    { const int rcp = check_complete(c, "kpilqr_get_union_columns"); if (rcp) return rcp; }
    const int rc = prepare_union(c);
    if (rc) return rc;
    const size_t entries = (size_t)c->d.dof * c->kpu_total, count = entries * 3 * c->n;
    if (columns) {
        if (count > capacity_doubles) return set_err(c, KPILQR_ERR_ARG, "union columns capacity too small");
        KP_HIP(c, hipMemcpyAsync(columns, c->kpcu, count * 8, hipMemcpyDeviceToHost, c->stream));
    }
    { const int rcs = sync_and_report(c); if (rcs) return rcs; }
    return (int)entries;
}

const char *kpilqr_backward_variant(kpilqr_ctx *c) { return c ? variant_name(c->bwd_family, c->tiled_a6) : ""; }
const char *kpilqr_forward_variant(kpilqr_ctx *c) { return c ? variant_name(c->fwd_family, c->tiled_a6) : ""; }

// What the last backward (which = 0) / forward (which = 1) launch of this context WAS: "<variant>" for the materialising
// families; for the fused sweeps "<variant>:<waves>:<columns>:<lists>[:ru0][:rxc][:slopes]" with
//   waves    w1 one wavefront per trajectory | pair | triple | pairh
//   columns  raw: the backward sweep differenced the key-point ordered payload itself | kpc: read from the column store
//   lists    uni: every DoF of a trajectory has the same key-point list (the straight-line crossing forms ran) | ragged
// and ":union" at the end when the launch ran on the union store of KPILQR_FLAG_UNION_KEYPOINTS (then `lists` is the union's: uni).
// The `lists` token is decided on the device (the host never needs it otherwise): this call reads the flag back, i.e. it
// waits for the context's stream.
// which = 2: the linearisation stage (a2 + a4) of the last kpilqr_fd_interpolate / kpilqr_iterate / kpilqr_iterate_streamed:
//   fd_kp_interpolate | kp_columns_interpolate (one pass, linearise.hip) | fd_difference+interpolate | in_sweep (fused context) |
//   kp_union (fused context, sweeps on the union store)
// ":subset" comes last where the launch was a listed one (kpilqr_backward_partial, kpilqr_forward_linear_partial, kpilqr_iterate_partial):
// the tokens before it are the form the list's length chose.
// which = 3: how the last forward launch scored its steps: "pair2" one r_x product per two steps (the uniform one-wave form with the
// constant Jacobian and n_alpha <= 8: FusedLaunch::pair2; uniform lists are the device's word, so this waits like which = 1) |
// "step" every step its own, i.e. every other launch; "" while the last forward call has launched nothing (none yet, or it was refused
// before its launch: FusedLaunch::fwd_ran, which travels with last_fwd -- a streamed iteration's chunk views hand it back with the plan);
// "?" where the flag cannot be read back (which = 1 then ends in ":?").
const char *kpilqr_last_launch(kpilqr_ctx *c, int which)
{
    if (c && which == 2) return c->last_linearise;
    if (c && which == 3) {
        const FusedLaunch &p = c->last_fwd;
        if (!p.fwd_ran) return "";
        if (!p.pair2) return "step";
        int uni = 0;
        if (hipSetDevice(c->d.device) != hipSuccess || (c->pipe_dirty && join_pipeline(c) != KPILQR_OK) ||
            hipMemcpyAsync(&uni, p.uni_on_union ? c->kpu_uniform : c->kp_uniform, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) return "?";
        return uni ? "pair2" : "step";
    }
    if (!c || which < 0 || which > 1) return "";
    std::string &out = c->launch_desc[which];
    const FusedLaunch &p = which == 0 ? c->last_bwd : c->last_fwd;
    out = variant_name(which == 0 ? c->bwd_family : c->fwd_family, c->tiled_a6);
    if (p.waves == Waves::none) {
        if (c->fused) { out += ":none"; return out.c_str(); }
        // the two-tile forward sweep on materialised tiles: one wave per row tile, or state / cost wave groups (small batches)
        // (a listed launch chose by its own width)
        Ctx w = *c;
        if (c->last_width[which] >= 0) w.d.batch = c->last_width[which];
        if (which == 1 && c->fwd_family == Family::tiled && !c->tiled_a6 && forward_tiled_sc_selected(&w)) out += ":state_cost_waves";
        if (c->last_width[which] >= 0) out += ":subset";
        return out.c_str();
    }
    int uni = 0;
    // (a launch on the union store read the union's flag, not the one of the caller's lists)
    if (hipSetDevice(c->d.device) != hipSuccess || (c->pipe_dirty && join_pipeline(c) != KPILQR_OK) ||
        hipMemcpyAsync(&uni, p.uni_on_union ? c->kpu_uniform : c->kp_uniform, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { out += ":?"; return out.c_str(); }
    static const char *const wname[] = {"", "w1", "pair", "triple", "pairh"};      // by Waves
    out += ":"; out += wname[(int)(uni ? p.waves : p.waves_ragged)];
    // (the raw launch sequence differences inside the sweep for uniform sets only: per-DoF lists take k_fd_kp_difference and
    // the plain sweep, launched behind it -- unless KPILQR_FUSED_UNI=0 forces the general raw form, one wave per trajectory)
    if (which == 0) out += (p.raw && (uni || (c->tune.fused_uni == 0 && p.waves == Waves::w1))) ? ":raw" : ":kpc";
    out += uni ? ":uni" : ":ragged";
    if (p.ru0) out += ":ru0";
    if (p.rxc) out += ":rxc";
    if (!uni && p.slopes) out += ":slopes";
    if (p.uni_on_union) out += ":union";
    if (c->last_width[which] >= 0) out += ":subset";
    if (c->embed.on) out += ":emb" + std::to_string(c->n) + "x" + std::to_string(c->d.m);      // (always last: the carrier's n' x m')
    return out.c_str();
}

}  // extern "C"
