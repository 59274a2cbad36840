/*
 * trackdlo_hip.h -- C ABI of the MI355X (gfx950) implementation of TrackDLO's per-frame EM
 * registration path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/Eigen/torch types.  Every entry
 * point names the reference interface it replaces (paths relative to the RMDLO/trackdlo tree).
 * All matrices are COLUMN-MAJOR doubles, the in-memory layout of Eigen::MatrixXd, so
 * `X.data()` / `Y.data()` of the reference's arguments can be passed straight through:
 *   X : N x 3, leading dimension N   (x[0..N) y[0..N) z[0..N))
 *   Y : M x 3, leading dimension M
 *
 * Error convention: functions return 0 on success or a negative TDLO_E_* code and never throw;
 * tdlo_last_error() returns a human-readable message for the last failure on that context.
 * (The reference path has no error channel at all: cpd_lle only returns `converged`,
 * trackdlo/src/trackdlo.cpp:433-440, which tracking_step discards, :927/:998.)
 *
 * Threading: a context is bound to one GPU and one HIP stream and is NOT thread-safe, matching the
 * reference's single-threaded use (ros::spin(), trackdlo/src/trackdlo_node.cpp:643).
 *
 * There is no CPU fallback: every entry point fails with TDLO_E_NO_DEVICE when no gfx950 device
 * is usable.
 */
#ifndef TRACKDLO_HIP_H
#define TRACKDLO_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* Counts INCOMPATIBLE changes of this interface: a changed signature, structure layout or meaning.  Entry points that are only added (the cloud and
 * image views, tdlo_sort_pts, tdlo_tracker_initialize_from_cloud, ...) leave it alone: a caller built against an earlier header of the same version
 * runs unchanged, and a caller that needs a newer entry point finds out by looking the symbol up. */
#define TDLO_ABI_VERSION 3

enum {
    TDLO_OK = 0,
    TDLO_E_NO_DEVICE = -1,   /* no usable HIP device / kernel image */
    TDLO_E_INVALID = -2,     /* bad argument (M < 4 or M > 1024, N <= 0, bad slot, ...) */
    TDLO_E_HIP = -3,         /* HIP runtime error, see tdlo_last_error */
    TDLO_E_EMPTY = -4,       /* the prune (trackdlo.cpp:177-195) removed every point */
    TDLO_E_NUMERIC = -5,     /* non-finite sigma2 / Y or singular system encountered */
    TDLO_E_TRAVERSE = -6,    /* traverse_euclidean would read out of bounds in the reference */
    TDLO_E_EXCHANGE = -7     /* N-split: a peer's contribution did not arrive in time / RCCL reported an error */
};

/* tdlo_params.precision */
enum {
    TDLO_PREC_F32 = 0,       /* fp32 E-step (distances, membership, sums per 64-point tile), fp64 M-step */
    TDLO_PREC_F64 = 1        /* fp64 everywhere */
};

typedef struct tdlo_ctx tdlo_ctx;

typedef struct {
    int device;              /* HIP device ordinal */
    int max_frames;          /* number of frame slots (>= 1); slots are independent clouds/trackers */
    int max_points;          /* initial per-slot capacity in points (grown on demand) */
    int max_nodes;           /* initial capacity in nodes (grown on demand) */
    int estep_blocks;        /* 0 = auto; otherwise workgroups per frame for the E-step */
} tdlo_config;

/* Arguments of trackdlo::cpd_lle after (X_orig, Y, sigma2): trackdlo/include/trackdlo.h:80-94. */
typedef struct {
    double beta;
    double lambda;
    double lle_weight;
    double mu;
    int max_iter;                 /* reference default 30 */
    double tol;                   /* reference default 1e-4 */
    int include_lle;              /* reference default true */
    double alpha;                 /* reference default 0 */
    double k_vis;                 /* reference default 0 */
    double visibility_threshold;  /* reference default 0.01 */
    int precision;                /* TDLO_PREC_*; not in the reference (which is fp64 on the CPU) */
} tdlo_params;

typedef struct {
    int iters;            /* EM iterations executed (the reference only logs this, trackdlo.cpp:426) */
    int converged;        /* return value of trackdlo::cpd_lle */
    int n_kept;           /* N after the prune, trackdlo.cpp:195 */
    int status;           /* 0, or TDLO_E_NUMERIC / TDLO_E_EMPTY */
    double sigma2;        /* final sigma2 (also written through the in/out pointer) */
    float loop_ms;        /* HIP-event time of the EM loop body on the context's stream (trackdlo.cpp:275-438); 0 unless tdlo_set_timing(ctx, 1) */
    float total_ms;       /* HIP-event time of the whole device-side call (prune + setup + loop + readback); 0 unless tdlo_set_timing(ctx, 1) */
    double host_ms;       /* host wall time of the call including uploads and the final synchronise */
    int mstep_retries;    /* iterations whose dense multi-workgroup elimination (a comparator / fall-back M-step, see tdlo_cpd_lle_resident) ran into
                           * the time limit of an inter-workgroup hand-off and were redone by the one-workgroup elimination (normally 0) */
    int sort_reused;      /* 1: this registration reused the slot's pruned, node-sorted cloud of the previous one (same cloud, same nodes, same
                           * precision: tdlo_set_sort_reuse) and skipped the prune of trackdlo.cpp:177-195 -- identical results; 0: it pruned;
                           * 2 (tdlo_tracker_tracking_step's main registration, every node visible): as 1, and its node-side set-up had been done
                           * by the pre-processing registration's prologue as well -- it started at its first E-step (TDLO_PAIR_SETUP=0: never) */
    int band_retry;       /* 1: the banded LLE M-step met a non-positive pivot (or a non-finite sigma2; in fp64 mode also a sigma2 computed from the
                           * data that is too large for the banded form to hold 1e-9 m, see tdlo_debug_band_retries) and the call was repeated on
                           * the dense pivoted eliminations, whose result this is (the reference's solver is a general one, trackdlo.cpp:415) */
} tdlo_stats;

/* ---- context ------------------------------------------------------------------------------- */
int tdlo_abi_version(void);
int tdlo_device_count(void);
void tdlo_default_config(tdlo_config *cfg);
/* Creates a context on cfg->device.  Replaces nothing in the reference (it has no device state);
 * it owns what `class trackdlo`'s members own (trackdlo/include/trackdlo.h:104-121) plus device buffers. */
tdlo_ctx *tdlo_create(const tdlo_config *cfg, int *err);
void tdlo_destroy(tdlo_ctx *ctx);
const char *tdlo_last_error(const tdlo_ctx *ctx);
/* raw hipStream_t of the context (for callers that time or order work on it) */
void *tdlo_stream(tdlo_ctx *ctx);
int tdlo_synchronize(tdlo_ctx *ctx);

/* ---- EM registration ----------------------------------------------------------------------- */
/* Uploads a point cloud into frame slot `slot` (H2D copy, stays resident in HBM).
 * Replaces the by-value `MatrixXd X_orig` argument of cpd_lle / tracking_step (trackdlo.h:80, :96). */
int tdlo_set_cloud(tdlo_ctx *ctx, int slot, const double *X, int N);

/* ---- clouds as they arrive: float32 or float64, any strides, host or device memory ------------- */
/* A view of N points somewhere in memory; nothing is copied to build one.  The reference's own cloud is float (pcl::PointXYZRGB: x, y, z at a
 * 32-byte point stride; widened and transposed on the host at trackdlo_node.cpp:242): view_of(&points[0].x, 8).  float -> double is exact, so a
 * cloud imported through a view is, bit for bit, what tdlo_set_cloud makes of the widened column-major copy. */
enum { TDLO_F32 = 0, TDLO_F64 = 1 };                        /* tdlo_cloud_view.dtype */
enum { TDLO_MEM_AUTO = 0, TDLO_MEM_HOST = 1, TDLO_MEM_DEVICE = 2 };   /* tdlo_cloud_view.location */
enum { TDLO_VIEW_ASYNC = 1 };                               /* tdlo_cloud_view.flags */
typedef struct {
    const void *data;          /* address of x of point 0 */
    int dtype, location;
    long long stride_point;    /* in ELEMENTS: component c of point n is element n*stride_point + c*stride_comp */
    long long stride_comp;     /* signed; packed row-major N x 3: (3, 1); PCL PointXYZ / XYZRGB: (4, 1) / (8, 1); column-major with leading dimension ld: (1, ld) */
    void *ready_stream;        /* device sources: hipStream_t whose work so far produces the data; NULL = the data is ready */
    int flags;
} tdlo_cloud_view;
/* Whether (v, N) describes a cloud: TDLO_E_INVALID for a null view or null data, N <= 0, an unknown dtype, location or flag bit, stride_point == 0
 * with N > 1, stride_comp == 0, data not aligned to its element size, an extent that does not fit 64-bit byte offsets.  Negative strides are legal
 * (a reversed view is a cloud).  Needs no context and no GPU; every call below that takes a view runs it first. */
int tdlo_cloud_view_check(const tdlo_cloud_view *v, int N);
/* The bytes the view addresses, relative to v->data: [*lo_bytes, *hi_bytes), from the first byte of its lowest element to one past the last byte of
 * its highest.  The library never reads a byte outside them, with any load. */
int tdlo_cloud_view_extent(const tdlo_cloud_view *v, int N, long long *lo_bytes, long long *hi_bytes);
/* tdlo_set_cloud from a view: the slot's resident cloud becomes the widened, column-major copy of the view (one kernel, k_cloud_import,
 * csrc/tdlo_import.hip; non-finite values are widened as (double) widens them -- the prune drops such points).
 *   location  TDLO_MEM_AUTO asks hipPointerGetAttributes; a pointer the runtime does not know is host memory.  Device memory of another GPU:
 *             TDLO_E_INVALID.  Managed and caller-pinned memory is treated as host memory and copied; no kernel dereferences it.
 *   host source    x, y, z are packed in the source precision into the context's pinned staging buffer (12 bytes per float point) and widened by the
 *             kernel, which reads that block in place over PCIe (TDLO_VIEW_INPLACE=0, read when the context is made: copied to the device first,
 *             the comparator).  The caller's memory is theirs again when the call returns.
 *   device source  the kernel reads the caller's memory in place.  The call returns after the import has finished; with TDLO_VIEW_ASYNC it is only
 *             enqueued on tdlo_stream(ctx), and the source must stay valid and unchanged until the caller's next call that waits for that stream
 *             (any registration, tdlo_get_cloud or tdlo_synchronize).  ready_stream: an event recorded on it makes the context's stream wait for
 *             the work that produces the data -- no host wait. */
int tdlo_set_cloud_view(tdlo_ctx *ctx, int slot, const tdlo_cloud_view *v, int N);
/* Copies the slot's resident cloud as it stands -- whatever tdlo_set_cloud, tdlo_set_cloud_view, tdlo_depth_to_cloud or a tracker frame left there
 * (what the node publishes on /trackdlo/filtered_pointcloud, trackdlo_node.cpp:480-484): n x 3 column-major, leading dimension n; *n_out = n.
 * x_capacity < n: TDLO_E_INVALID with *n_out set.  Waits for the context's stream. */
int tdlo_get_cloud(tdlo_ctx *ctx, int slot, double *X_out, int x_capacity, int *n_out);

/* trackdlo::cpd_lle (trackdlo/src/trackdlo.cpp:161-441) on the cloud resident in `slot`.
 *   Y        in/out  M x 3 column-major           (MatrixXd& Y)
 *   sigma2   in/out                                (double& sigma2; 0 => initialised as at :271-273)
 *   priors   K x 4 row-major [idx, x, y, z]        (std::vector<MatrixXd> correspondence_priors)
 *   visible_nodes, n_vis                           (std::vector<int> visible_nodes)
 *   H_override optional M x M column-major matrix used in place of the LLE regulariser
 *              H = (I-L)^T (I-L) of :236-237 (whose weights are numerically ill-defined).
 * Returns 0 or an error; stats->converged carries the reference's bool result.
 * Chains of 4 .. 1024 nodes (more: TDLO_E_INVALID).  Which kernel solves the M-step (trackdlo.cpp:392-437), by default, for chains of up to 512 nodes
 * (beyond 512: the one-direction smoother k_mstep_chain_long without the LLE term, the one-workgroup dense elimination with it):
 *   include_lle == 0  the chain smoother (csrc/tdlo_mstep_chain.hip: the same linear system in O(M) through the state-space form of
 *                     the kernel G, one workgroup per frame);  lambda == 0 or TDLO_MSTEP=dense: the dense eliminations k_mstep_fast
 *                     (up to 60 nodes) / k_mstep_mcu (one workgroup per 16 rows) -- comparators of the tests;
 *   include_lle == 1  the banded L D L^T in the chain's state (csrc/tdlo_mstep_band.hip, O(M)) when no two consecutive nodes are closer
 *                     than about a millimetre and H is banded and symmetric (the library's own always is); otherwise, after a
 *                     non-positive pivot (stats->band_retry), or with TDLO_MSTEP_LLE=dense: the dense pivoted eliminations
 *                     k_mstep_fast (up to 64 nodes) / k_mstep (up to 128) / k_mstep_pivot_mcu (beyond; TDLO_MSTEP_LLE=1wg keeps it in
 *                     one workgroup).  stats->mstep_retries counts time-outs of the multi-workgroup forms only.
 * Sorted-cloud reuse: the prune (:177-195) and the sort by nearest node depend on the cloud and on the incoming nodes only.  A call
 * whose Y equals, bit for bit, the Y of the previous registration of the same slot in the same precision, with the slot's cloud
 * untouched in between (no tdlo_set_cloud / tdlo_depth_to_cloud / N-split on it), reuses that result instead of pruning again
 * (stats->sort_reused = 1; identical output).  In the reference this happens for the two registrations of a tracking_step whose nodes
 * are all visible (:913-927 and :998 start from the same Y_).  tdlo_set_sort_reuse(ctx, 0) or TDLO_REUSE_SORT=0 turn it off. */
int tdlo_cpd_lle_resident(tdlo_ctx *ctx, int slot, double *Y, int M, double *sigma2,
                          const tdlo_params *params, const double *priors, int K,
                          const int *visible_nodes, int n_vis, const double *H_override,
                          tdlo_stats *stats);

/* Same, taking the cloud from host memory like the reference signature does:
 * tdlo_set_cloud(slot 0) followed by tdlo_cpd_lle_resident. */
int tdlo_cpd_lle(tdlo_ctx *ctx, const double *X, int N, double *Y, int M, double *sigma2,
                 const tdlo_params *params, const double *priors, int K,
                 const int *visible_nodes, int n_vis, const double *H_override,
                 tdlo_stats *stats);

/* Batched form: F independent registrations (slots 0..F-1, clouds already resident), executed
 * concurrently on the GPU.  Arrays are indexed by frame; Y is F consecutive M x 3 blocks; priors/
 * visible_nodes are shared by all frames (pass K = 0 / n_vis = 0 for none).  No reference
 * counterpart: the reference processes one frame per call (BASELINE.json configs[2]).
 * Batches of 8 or more frames run as groups of frames on streams owned by the context (2 groups from 8 frames, 4 from 16, 3 from
 * 28 -- about what the GPU holds at once per E-step launch), staggered by one E-step, so that one group's M-step (one workgroup per
 * frame) overlaps another group's E-step; every frame's result is the same, bit for bit, as from tdlo_cpd_lle_resident
 * (environment TDLO_BATCH_STREAMS=n forces n groups, 1: one stream).  The sorted cloud is reused only when EVERY frame of the batch
 * can reuse its own.  The call returns after all streams have drained. */
int tdlo_cpd_lle_batch(tdlo_ctx *ctx, int F, double *Y, int M, double *sigma2,
                       const tdlo_params *params, const double *priors, int K,
                       const int *visible_nodes, int n_vis, const double *H_override,
                       tdlo_stats *stats /* F entries */);

/* The batch with per-frame arguments: frame i runs in slots[i] (distinct, any order; NULL: 0..F-1) with its own priors, visible set and H
 * (args == NULL: none for any frame).  Everything else is as in tdlo_cpd_lle_batch; F == 1 is the one-frame route.  Per frame: priors, K, n_vis (hence the
 * visibility weighting of trackdlo.cpp:358) and H_override.  Per batch: the E-step kernel, the replica rows of the sums, the sort reused only when every frame
 * can reuse its own, the dense LLE kernels when one frame cannot take the banded solve.  The E-step is instantiated per launch with or without the
 * visibility weights: frames that disagree there run as two batches one behind the other.
 * Bits: with the same E-step kernel on both sides (contexts made under TDLO_ESTEP2=0, or =1) and, with the LLE term, every frame on the banded solve, each
 * frame's nodes, sigma2 and counts are those of tdlo_cpd_lle_resident with the same arguments, bit for bit; otherwise within the gates DESIGN.md 4 states
 * between k_estep and k_estep2 (1e-7 m, 1e-5 relative in sigma2) and between the banded and the dense solve.
 * Every frame's stats are filled (stats[i].status: that frame's verdict); the call returns the first non-zero one. */
typedef struct { const double *priors; int K; const int *visible_nodes; int n_vis; const double *H_override; } tdlo_frame_args;
int tdlo_cpd_lle_batch_each(tdlo_ctx *ctx, int F, const int *slots /* distinct; NULL: 0..F-1 */, double *Y, int M, double *sigma2,
                            const tdlo_params *params, const tdlo_frame_args *args /* F entries; NULL: none */, tdlo_stats *stats /* F */);

/* ---- N-split building blocks (BASELINE.json configs[3]) --------------------------------------- */
/* When one frame's cloud is split over several GPUs, each rank holds a shard in slot 0 and the
 * host interleaves these calls with an all-reduce (SUM) of the packed buffer
 *   sums[0..M) = P1, sums[M..4M) = R = PX - P1 y (column-major M x 3, residual w.r.t. the current nodes,
 *   which are identical on every rank), sums[4M] = Q, sums[4M+1] = N_kept
 * and, when visibility weighting is active, an all-reduce (MIN) of dmin[M].
 * They expose the halves of one iteration of trackdlo.cpp:275-438. */
int tdlo_split_begin(tdlo_ctx *ctx, const double *Y, int M, double sigma2, const tdlo_params *params,
                     const double *priors, int K, const int *visible_nodes, int n_vis,
                     const double *H_override, double *init /* out: [n_kept_local, sum_d2_local] */);
int tdlo_split_set_global(tdlo_ctx *ctx, double n_kept_global, double sum_d2_global);
int tdlo_split_dmin(tdlo_ctx *ctx, double *dmin_sq /* out M, local */);
int tdlo_split_estep(tdlo_ctx *ctx, const double *dmin_sq_global /* in M or NULL */, double *sums /* out 4M+2 */);
int tdlo_split_mstep(tdlo_ctx *ctx, const double *sums_global /* in 4M+2 */, int *done /* out */);
int tdlo_split_end(tdlo_ctx *ctx, double *Y, double *sigma2, tdlo_stats *stats);
/* Leaves a split registration without results (e.g. after the global kept-point count came back 0): drains the stream,
 * unbinds the exchange buffers, so that the context can begin the next registration. */
int tdlo_split_abort(tdlo_ctx *ctx);

/* Device-resident exchange (the form the 8-GPU run uses): the two buffers the ranks all-reduce live in DEVICE memory
 * owned by the caller -- e.g. a tensor handed to RCCL -- and the calls below only enqueue work on the context's stream
 * (tdlo_stream), so one EM iteration is   dmin_enqueue, all-reduce MIN d_dmin, estep_enqueue, all-reduce SUM d_sums,
 * mstep_enqueue   with every collective issued on (or ordered after) that stream and NO host synchronisation; the
 * stopping rule is evaluated on the device and read with tdlo_split_poll every few iterations (kernels of a finished
 * registration are no-ops, all ranks see the same flag because they solve the same system).
 *   d_dmin: M doubles, per-node minimum SQUARED distance (1e300 where a shard holds no point); only touched when
 *           visibility weighting is active.   d_sums: 4M+2 doubles, layout as above.
 * Bind before tdlo_split_begin; bind (NULL, NULL) to return to the host-buffer calls. */
int tdlo_split_bind_exchange(tdlo_ctx *ctx, double *d_dmin /* device, M */, double *d_sums /* device, 4M+2 */);
int tdlo_split_dmin_enqueue(tdlo_ctx *ctx);    /* local dmin -> d_dmin */
int tdlo_split_estep_enqueue(tdlo_ctx *ctx);   /* d_dmin (global) -> E-step on the shard -> local sums -> d_sums */
int tdlo_split_mstep_enqueue(tdlo_ctx *ctx);   /* d_sums (global) -> M-step (:392-437), identical on every rank */
int tdlo_split_poll(tdlo_ctx *ctx, int *done, int *iters);   /* synchronises the stream */

/* ---- the split registration driven from C++ (no torch, no Python in the loop) -------------------------------------- */
/* One whole trackdlo::cpd_lle (trackdlo.cpp:161-441) with the cloud split over the ranks: every rank holds its shard in slot 0
 * (tdlo_set_cloud / tdlo_depth_to_cloud) and calls this with the same Y, sigma2 and parameters; every rank returns the same
 * Y, sigma2, iteration count (the replicated M-step solves the same system from the same bits).  stats->n_kept is the
 * shard's count.  Two forms:
 *   nccl_comm != NULL  an RCCL communicator (ncclComm_t) over the ranks: per iteration the all-reduce MIN of dmin[M]
 *       (visibility weighting only) and the all-reduce SUM of the 4M+2 sums, issued by this library on the context's stream
 *       between its kernels (librccl is bound at run time: an RCCL already mapped into the process -- PyTorch's -- is used,
 *       else $TDLO_RCCL_LIB / tdlo_rccl_load, else the system's); any chain length.
 *   nccl_comm == NULL  the ONE-SHOT EXCHANGE bound with tdlo_xch_bind: no collective at all.  Every rank writes its minima /
 *       sums straight into every peer's inbox (peer stores: xGMI on a multi-GPU node) and raises a flag; the last workgroup of
 *       the min-distance kernel and the one-workgroup M-step wait for the R flags in their own inbox and reduce the R
 *       contributions in rank order.  One EM iteration is the three kernels of the unsplit loop, no launch in between.
 *       Any chain length (the one-workgroup M-steps carry the exchange: the chain smoother, and with the LLE term the banded
 *       L D L^T; a registration whose LLE system takes the dense eliminations -- coincident nodes, an H_override that is not banded --
 *       only up to 64 nodes); up to 8 ranks.  A rank that is more than 2 s behind its peers (or gone) makes the waiting kernels give up:
 *       TDLO_E_EXCHANGE on the ranks that waited.  A rank whose own shard fails (TDLO_E_NUMERIC from the E-step's range check) raises its
 *       flag with an error mark: its peers leave the same iteration with TDLO_E_NUMERIC instead of waiting out the limit.  Arguments are validated before anything is exchanged; a shard that loses every point
 *       to the prune still takes part (it contributes zeros).  A group of ONE rank has nobody to exchange with: the per-iteration
 *       exchange is skipped (the plain call's kernels and bits); TDLO_XCH_SELF=1 (read per call) makes it write to and read from its
 *       own inbox like a rank of a larger group -- what the exchange itself costs on one GPU (bench.py, tests).
 * The stopping rule is evaluated on the device and read after iterations 1, 2, 4, 8, 12, ... (tol > 0).
 * With the LLE term, a banded solve that meets a non-positive pivot is repeated on the dense pivoted kernels by all ranks together
 * (stats->band_retry), as tdlo_cpd_lle_resident does; in the one-shot form only for chains of up to 64 nodes (longer: TDLO_E_NUMERIC). */
int tdlo_split_run(tdlo_ctx *ctx, void *nccl_comm, double *Y, int M, double *sigma2, const tdlo_params *params,
                   const double *priors, int K, const int *visible_nodes, int n_vis, const double *H_override, tdlo_stats *stats);
/* One-shot exchange set-up.  tdlo_xch_create allocates this rank's inbox (device memory, zeroed; tdlo_xch_bytes bytes) for
 * `nranks` ranks and chains up to `max_nodes` nodes.  Ranks in other processes export / open it as a HIP IPC handle (64
 * bytes, carried by whatever the host application uses to bootstrap: MPI, a file, a socket); ranks in one process pass the
 * pointers directly.  tdlo_xch_bind takes the device pointers of ALL ranks' inboxes, valid on this context's device, own
 * inbox at [rank]; nranks == 0 unbinds. */
size_t tdlo_xch_bytes(int nranks, int max_nodes);
int tdlo_xch_create(tdlo_ctx *ctx, int nranks, int max_nodes, void **inbox);
int tdlo_xch_ipc_export(tdlo_ctx *ctx, void *handle64);
int tdlo_xch_ipc_open(tdlo_ctx *ctx, const void *handle64, void **peer_inbox);
int tdlo_xch_bind(tdlo_ctx *ctx, int rank, int nranks, void *const *inboxes);
/* Whether this context's GPU can map memory of `peer_device` (hipDeviceCanAccessPeer; 1 for its own device): what a rank asks before it
 * opens a peer's inbox.  Failures of the exchange's set-up that are properties of the node, not errors of the caller -- no fine-grained
 * device memory for the inbox (tdlo_xch_create with more than one rank), an inbox that cannot be mapped (tdlo_xch_ipc_open,
 * tdlo_xch_bind) -- come back as TDLO_E_EXCHANGE: the ranks then agree (e.g. a MIN all-reduce of "set up") to use the RCCL form. */
int tdlo_xch_can_access(tdlo_ctx *ctx, int peer_device, int *can);
/* RCCL bootstrap for hosts that have no communicator of their own: rank 0 makes the 128-byte ncclUniqueId and hands it to
 * the other ranks; every rank then creates its communicator (owned by the context, destroyed with it).  tdlo_rccl_load
 * names the librccl to bind (NULL: search as described above); returns 0 when RCCL is usable. */
int tdlo_rccl_load(const char *path);
int tdlo_rccl_unique_id(void *id128);
int tdlo_rccl_comm_init(tdlo_ctx *ctx, int nranks, int rank, const void *id128, void **comm_out);
/* ncclCommCount / ncclCommUserRank of a communicator (any ncclComm_t of the RCCL this library is bound to): what a rank reports
 * about the group it really is in. */
int tdlo_rccl_comm_count(void *comm, int *nranks, int *rank);

/* ---- tracker object: class trackdlo (trackdlo/include/trackdlo.h:53-130) ---------------------- */
typedef struct tdlo_tracker tdlo_tracker;

/* trackdlo::trackdlo(int num_of_nodes, double visibility_threshold, double beta, double lambda,
 *   double alpha, double k_vis, double mu, int max_iter, double tol, double beta_pre_proc,
 *   double lambda_pre_proc, double lle_weight)  -- trackdlo.cpp:30-59.  Uses slot `slot` of ctx. */
tdlo_tracker *tdlo_tracker_create(tdlo_ctx *ctx, int slot, int num_of_nodes, double visibility_threshold,
                                  double beta, double lambda, double alpha, double k_vis, double mu,
                                  int max_iter, double tol, double beta_pre_proc,
                                  double lambda_pre_proc, double lle_weight);
/* trackdlo::trackdlo(int num_of_nodes) defaults -- trackdlo.cpp:10-28 */
tdlo_tracker *tdlo_tracker_create_default(tdlo_ctx *ctx, int slot, int num_of_nodes);
void tdlo_tracker_destroy(tdlo_tracker *t);
int tdlo_tracker_set_precision(tdlo_tracker *t, int precision);
/* trackdlo::initialize_nodes (trackdlo.cpp:83-86) */
int tdlo_tracker_initialize_nodes(tdlo_tracker *t, const double *Y_init /* M x 3 */);
/* trackdlo::initialize_geodesic_coord (trackdlo.cpp:77-81; appends, like the reference) */
int tdlo_tracker_initialize_geodesic_coord(tdlo_tracker *t, const double *coord, int n);
/* The implicit copy assignment of class trackdlo (trackdlo/include/trackdlo.h:104-121 has no user-defined one: every member is
 * copied -- Y_, guide_nodes_, sigma2_, the eleven parameters, geodesic_coord_, correspondence_priors_).  The ROS node relies on
 * it once (trackdlo_node.cpp:131 assigns a configured object to the file-scope default-constructed one, :54).  Both trackers
 * must have the same number of nodes; dst keeps its own context and slot. */
int tdlo_tracker_copy_state(tdlo_tracker *dst, const tdlo_tracker *src);
/* trackdlo::get_sigma2 / set_sigma2 (trackdlo.cpp:61-63, :88-90) */
double tdlo_tracker_get_sigma2(const tdlo_tracker *t);
void tdlo_tracker_set_sigma2(tdlo_tracker *t, double sigma2);
/* trackdlo::get_tracking_result (trackdlo.cpp:65-67): copies M x 3 */
int tdlo_tracker_get_tracking_result(const tdlo_tracker *t, double *Y_out);
/* trackdlo::get_guide_nodes (trackdlo.cpp:69-71): returns row count, copies rows x 3 */
int tdlo_tracker_get_guide_nodes(const tdlo_tracker *t, double *out, int max_rows);
/* trackdlo::get_correspondence_pairs (trackdlo.cpp:73-75): returns K, copies K x 4 row-major */
int tdlo_tracker_get_correspondence_pairs(const tdlo_tracker *t, double *out, int max_rows);
/* trackdlo::tracking_step (trackdlo.cpp:900-999).  proj_matrix/img_rows/img_cols of the reference
 * signature are unused by its body and therefore not part of the ABI.  H_pre: optional override of
 * the pre-processing registration's LLE matrix (n_vis_ext x n_vis_ext).  stats may be NULL;
 * otherwise stats[0] = pre-processing registration (:927), stats[1] = main registration (:998). */
/* X == NULL: use the cloud already resident in the tracker's slot (tdlo_set_cloud / tdlo_depth_to_cloud); N ignored.
 *
 * How a frame is run (nothing of this changes a bit of any result; each item has an environment switch, read when the context is made, that
 * turns it off -- the comparators of tests/test_direct_path_gpu.py; tdlo_debug_route_count counts how often each was taken):
 *  - X (up to 16 384 points) is copied into the context's pinned staging buffer and read from THERE by the first kernel of the frame, which
 *    also puts it in the slot's device buffer: no host-to-device copy on the stream (TDLO_DIRECT_CLOUD=0: hipMemcpyAsync as tdlo_set_cloud).
 *    X is the caller's again when the function returns, as before.
 *  - With every node visible (n_vis_ext == num_of_nodes) both registrations start from the same nodes Y_ on the same cloud
 *    (:913-927 and :998).  The main registration then (a) reuses the pre-processing registration's pruned, sorted cloud (tdlo_set_sort_reuse),
 *    (b) has its node-side set-up done by one more workgroup of the pre-processing registration's prologue (TDLO_PAIR_SETUP=0: a kernel of
 *    its own), (c) starts from the sums of the pre-processing registration's first E-step instead of repeating it -- same cloud, nodes,
 *    sigma2, mu, no visibility term, and the sums are integers: the same bits (TDLO_PAIR_SUMS=0) -- and (d) has its first M-step
 *    launched right behind the pre-processing registration's first iteration; it waits on the device for the priors that the host
 *    forms from that registration's result (:929-995) and leaves untouched if that registration needs more iterations or ends on an
 *    error (TDLO_SPEC_MSTEP=0: launched when the priors exist).  stats[1].sort_reused is 2 on such a frame.
 *  - With HIDDEN nodes (n_vis_ext < num_of_nodes) the registrations start from different node sets and share nothing -- but the main
 *    registration's prune, sort, set-up, per-node minimum distances and first E-step (:177-389 of the :998 call) depend on nothing the
 *    pre-processing registration produces.  They are launched on a second stream, into a second set of buffers of the context (the cloud
 *    is read from the same pinned staging buffer), as soon as the pre-processing registration's first iterations are on the first one,
 *    and run beside its iterations (6-7 with a stretch of the rope hidden); the first M-step waits behind them for the priors, as in (d),
 *    and the main registration stays on the second stream (TDLO_AHEAD=0: launched when the pre-processing registration has returned;
 *    tdlo_debug_route_count(ctx, 4)).  Such a frame does not leave the next frame's H behind (next item).  Clouds of up to 16 384 points,
 *    chains of up to 256 nodes.
 *  - The M-step that finishes the main registration also forms H = (I - L)^T (I - L) (:236-237) of the nodes it leaves behind, on the
 *    device, bit for bit what tdlo_calc_lle_regulariser gives (tdlo_debug_lle_band_device); the next frame's pre-processing registration
 *    uses it if it starts from exactly those nodes (every node visible, no H_pre) instead of waiting for the host's 6 x 6 factorisations
 *    (TDLO_LLE_NEXT=0).
 *  - Each registration enqueues as many iterations up front as the same registration took in the previous frame (1 .. 8) before the host
 *    looks at its state (trackdlo.cpp:424-428 is decided on the device; kernels of a finished registration are no-ops): consecutive frames
 *    take about the same number, and the GPU neither idles between iterations nor runs more than a no-op or two (TDLO_ITER_HINT=0: one).
 * A steady-state frame at production size (5 000 points, 45 nodes, both registrations converging in their first iteration) is then FOUR
 * kernels and no copy.  The calls of a context must come from one thread at a time (as for every entry point). */
int tdlo_tracker_tracking_step(tdlo_tracker *t, const double *X, int N,
                               const int *visible_nodes, int n_vis,
                               const int *visible_nodes_extended, int n_vis_ext,
                               const double *H_pre, tdlo_stats *stats);
/* tdlo_tracker_tracking_step with a view (above) in the place of X, N; everything behind the placing of the cloud is the same code, the same bits.
 *  - A HOST view of up to 16 384 points, where tdlo_tracker_tracking_step stages X in pinned memory: the host widens the view straight into that
 *    staging buffer (one pass over the points, where the memcpy stands), and the frame is the route described above -- four kernels and no copy in
 *    the steady state, stats[1].sort_reused == 2 (tdlo_debug_route_count 18).
 *  - A device view, or a larger cloud: tdlo_set_cloud_view enqueued without a host wait (a device source must stay valid until this call returns:
 *    the pre-processing registration waits for the stream), then the X == NULL route (tdlo_debug_route_count 17). */
int tdlo_tracker_tracking_step_view(tdlo_tracker *t, const tdlo_cloud_view *v, int N,
                                    const int *visible_nodes, int n_vis, const int *visible_nodes_extended, int n_vis_ext,
                                    const double *H_pre, tdlo_stats *stats);

/* ---- F trackers in one call ------------------------------------------------------------------------ */
/* trackdlo::tracking_step for F trackers of ONE context -- several ropes in a work cell, one rope seen by several cameras, many recorded sequences at
 * once -- on the clouds resident in the trackers' slots.  The steps are those of tdlo_tracker_tracking_step per tracker; the registrations run as
 * batches (tdlo_cpd_lle_batch_each): the pre-processing registrations one batch per distinct chain length n_vis_ext[i] (steady state: one; a group of
 * one takes the one-frame route), the priors per tracker on the host, then all main registrations as one batch of num_of_nodes nodes.  The single
 * tracker's short cuts (paired set-up, handed-over sums, the M-step launched ahead, the H left behind, the mailbox) do not apply to a batch.
 * Refused as a whole with TDLO_E_INVALID, before anything is touched, unless: all trackers share one context, their slots are distinct and hold a cloud,
 * num_of_nodes, precision and the eleven reference parameters are the same, nodes and geodesic coordinates are initialised, and every index list is in
 * range (visible_nodes_extended: 1 .. num_of_nodes indices).
 *   visible_nodes / n_vis, visible_nodes_extended / n_vis_ext   F pointers / F counts; visible_nodes may be NULL (nobody visible by distance)
 *   H_pre     NULL, or F entries each NULL or n_vis_ext[i]^2 doubles
 *   stats     NULL or 2 F entries: [2 i] pre-processing, [2 i + 1] main registration of tracker i
 *   rc_each   NULL or F codes.  A tracker whose step ends on TDLO_E_EMPTY, TDLO_E_TRAVERSE or TDLO_E_NUMERIC gets that code and is left as the single
 *             call leaves it on that error; the other trackers' steps complete.  The call returns the first non-zero code.
 * Bits: every tracker's nodes, sigma2, guide nodes, priors and counts are those of F tdlo_tracker_tracking_step calls when both sides run the same
 * E-step kernel (contexts made under TDLO_ESTEP2=0, or =1) and every pre-processing registration takes the banded solve; otherwise they lie within the
 * gates DESIGN.md 4 states between k_estep and k_estep2 (1e-7 m, 1e-5 relative in sigma2) and between the banded and the dense solve.
 * Fewer than THREE trackers are stepped one by one by the single call (same route, same cost, same bits on a same-kernel context): at production size
 * in steady state two trackers cost 0.128 ms as batches against 0.105 ms one by one, three 0.143 against 0.158 ms, 32 0.67 against 1.71 ms
 * (profiles/tracker_batch_ab.txt; TDLO_TRACKER_BATCH_MIN=n moves the crossover). */
int tdlo_tracker_tracking_step_batch(tdlo_tracker *const *trackers, int F,
                                     const int *const *visible_nodes, const int *n_vis,
                                     const int *const *visible_nodes_extended, const int *n_vis_ext,
                                     const double *const *H_pre /* NULL, or F entries each NULL or n_vis_ext[i]^2 */,
                                     tdlo_stats *stats /* NULL or 2 F: [2i] pre-processing, [2i+1] main */, int *rc_each /* NULL or F */);
/* The frame behind it: tdlo_visibility_prepass_batch of the trackers' current nodes against their resident clouds (visibility_threshold: the trackers'
 * own), the self-occlusion test per tracker where tdlo_tracker_set_self_occlusion switched it on, then tdlo_tracker_tracking_step_batch -- the bits of
 * tdlo_visibility_prepass + tdlo_tracker_tracking_step per tracker, under the conditions above.  A tracker without a visible node gets TDLO_E_EMPTY in
 * rc_each and is not touched; the others go on.  visible_nodes / visible_nodes_extended: F rows of num_of_nodes entries, n_vis / n_vis_ext: F counts;
 * any of them may be NULL.  stats / rc_each as above. */
int tdlo_tracker_frame_batch(tdlo_tracker *const *trackers, int F, double d_vis,
                             int *visible_nodes /* F x M or NULL */, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                             tdlo_stats *stats, int *rc_each);

/* ---- plain GMM-EM initial registration ------------------------------------ */
/* reg(pts, Y, sigma2, M, mu, max_iter), trackdlo/src/utils.cpp:21-82 (declared trackdlo/include/utils.h): M centroids
 * fitted to the cloud with the Euclidean membership only; Y (M x 3 column-major) and sigma2 are pure outputs (the
 * reference overwrites both, :24-29, :45).  Exactly max_iter iterations, no stopping rule, fp64.  M <= 890 (per-wave
 * accumulators in LDS; more is TDLO_E_INVALID).  pts == NULL: use the
 * cloud resident in `slot`.  A centroid that attracts no probability mass comes back NaN, as in the reference. */
int tdlo_reg(tdlo_ctx *ctx, int slot, const double *pts, int N, double *Y, double *sigma2, int M, double mu, int max_iter);

/* ---- chain order of unordered nodes, and a tracker started from its first cloud -------------------- */
/* MatrixXd sort_pts(MatrixXd Y_0), trackdlo/src/utils.cpp:95-170 (declared utils.h:26; prototype utils/tracking_test.py:174-229): reg returns its
 * centroids in no particular order; this puts them in chain order.  Node 0 is first; a minimum spanning tree is grown from it, each of the M - 1 rounds
 * taking the pair (a in the tree, b outside) of smallest non-zero squared distance -- fp64, (dx dx + dy dy) + dz dz with every product and sum
 * rounded, ties to the smallest a, then the smallest b -- and b enters the list by the reference's reverse / insertion bookkeeping (:134-157).
 * One workgroup, thread = node (k_sort_pts, csrc/tdlo_init.hip); 2 <= M <= 1024, anything else TDLO_E_INVALID.
 *   Y         M x 3 column-major, host memory.
 *   Y_sorted  M x 3 column-major: row i is row perm[i] of Y (may be Y itself; optional).
 *   perm      M ints (optional); the permutation is the reference's EXACTLY: the decisions compare identical fp64 values.
 *   coord     M doubles (optional): coord[0] = 0, coord[i] = coord[i - 1] + |Y_sorted[i] - Y_sorted[i - 1]|, added serially in chain order as
 *             trackdlo_node.cpp:135-141 and the prototype (:531-537) do -- what tdlo_tracker_initialize_geodesic_coord wants.
 * TDLO_E_NUMERIC, outputs untouched, the reason in tdlo_last_error: a non-finite coordinate; two nodes whose three coordinates are equal (as
 * values: -0.0 equals 0.0 -- the reference finds rows of its list by value and would confuse them); a round that finds no edge (every
 * remaining squared distance underflowed to zero or is infinite; the reference would repeat node 0). */
int tdlo_sort_pts(tdlo_ctx *ctx, const double *Y, int M, double *Y_sorted, int *perm, double *coord);
/* The same rule, outputs and verdicts in plain C++ on the host, no device and no context: the twin the CPU tests hold to the rule, and the comparator
 * route of tdlo_tracker_initialize_from_cloud. */
int tdlo_sort_pts_host(const double *Y, int M, double *Y_sorted, int *perm, double *coord);
/* The prototype's first-frame initialiser (utils/tracking_test.py:523-541): register(cloud, M, mu), sort_pts, cumulative segment lengths -- with M the
 * tracker's node count -- and the result installed as tdlo_tracker_initialize_nodes and tdlo_tracker_initialize_geodesic_coord would (trackdlo_node.cpp:131-146),
 * except that the coordinates REPLACE the tracker's instead of being appended.  This is NOT initialize.py's initialiser (skeleton, spline fit; skimage,
 * OpenCV, scipy), which stays out of scope: it is the one the E-step provides.
 *   X, N        the cloud (N x 3 column-major); X == NULL: the cloud resident in the tracker's slot, as tdlo_tracker_tracking_step does -- what
 *               tdlo_depth_to_cloud, tdlo_colour_depth_to_cloud, tdlo_frame_to_cloud_view, tdlo_cloud_view_voxel_grid or tdlo_set_cloud_view left
 *               there: such a cloud becomes a running tracker without visiting the host.
 *   mu, max_iter  reg's (the prototype calls 0.05, 100).
 *   sigma2_out  reg's sigma2 (optional).  The tracker's own sigma2 is left alone: the node sets nodes and coordinates only.
 * reg's whole loop and k_sort_pts, which reads reg's centroids where reg left them, are enqueued together: one wait, one read-back.
 * TDLO_INIT_SORT=host (read when the context is made): the centroids are read back and ordered by tdlo_sort_pts_host -- the comparator, the same bits
 * (tdlo_debug_route_count 25 / 26).  Errors leave the tracker EXACTLY as it was: TDLO_E_INVALID for fewer than 4 or more than 890 nodes (reg's limit),
 * N <= 0, an empty slot, bad mu / max_iter; TDLO_E_NUMERIC when a centroid came back NaN (it attracted no mass) or tdlo_sort_pts would refuse the centroids. */
int tdlo_tracker_initialize_from_cloud(tdlo_tracker *t, const double *X, int N, double mu, int max_iter, double *sigma2_out);
/* tdlo_set_cloud_view (enqueued without a host wait; a device source must stay valid until this call returns), then the X == NULL route above. */
int tdlo_tracker_initialize_from_cloud_view(tdlo_tracker *t, const tdlo_cloud_view *v, int N, double mu, int max_iter, double *sigma2_out);

/* ---- many trackers started in one call ------------------------------------------------------------- */
/* tdlo_reg, tdlo_sort_pts and tdlo_tracker_initialize_from_cloud for F frames at once.  A tracker's start is 2 + 2 max_iter launches of a few workgroups
 * each; here the F loops are the second grid dimension of the SAME 2 + 2 max_iter launches (k_reg_estep_batch / k_reg_mstep_batch, csrc/tdlo_reg_batch.hip:
 * every frame its own state and partial sums, no workgroup waits for another), k_sort_pts runs once with one workgroup per frame, and one upload, one
 * read-back and one wait serve them all.  All three work on the clouds RESIDENT in the slots -- what tdlo_set_cloud, tdlo_set_cloud_view,
 * tdlo_depth_to_cloud_batch / tdlo_tracker_frames_batch or the single cloud calls left there (a cloud tracking_step staged is flushed first).
 * Bits: for every frame reg's Y and sigma2, the permutation, the sorted nodes and the chain coordinate are the single calls' bit for bit, a centroid that
 * attracts no mass NaN in the same places; a single call made afterwards on the same context gives what it always gave.
 * Refused as a whole with TDLO_E_INVALID before anything is enqueued or touched (the reason in tdlo_last_error): F < 1 or a null pointer, trackers of
 * different contexts, a slot out of range or named twice, a slot without a cloud, node counts that differ, fewer than 4 or more than 890 nodes
 * (tdlo_reg_batch: M < 1; tdlo_sort_pts_batch: M outside 2 .. 1024), bad mu / max_iter.
 * One frame fails with TDLO_E_NUMERIC where the single call would (a NaN centroid, tdlo_sort_pts' three refusals): it gets the code in rc_each, its
 * tracker and its outputs stay exactly as they were, the other frames complete as if alone; the call returns the first non-zero code and
 * tdlo_last_error names that frame with the single call's reason.
 * Cost (profiles/init_batch_ab.txt; N = 5 000, M = 45, 100 iterations): two trackers 5.69 against 11.61 ms for two single calls, 32 trackers 11.79 against
 * 186.0 ms; with voxel-grid-sized clouds (N = 500) 32 trackers 5.31 against 167.8 ms.  One frame is level with the single call (5.72 against 5.81 ms).
 * TDLO_INIT_BATCH_MIN=n (read when the context is made): below n frames the call loops over the single calls -- the comparator; the default is 1, the
 * smallest F from which the batch launches won by the rule set before they were measured, so by default every call takes them.
 * tdlo_debug_route_count 36 / 37 count the frames of the two routes; TDLO_INIT_SORT=host applies as to the single call (the F centroid sets are read
 * back once and ordered by tdlo_sort_pts_host).
 *   tdlo_reg_batch        slots: F distinct slots; Y: F blocks of M x 3 column-major, sigma2: F -- pure outputs as tdlo_reg's.
 *   tdlo_sort_pts_batch   Y: F blocks of M x 3 column-major in host memory; Y_sorted / perm / coord: NULL or F blocks; rc_each: NULL or F codes.
 *   tdlo_tracker_initialize_from_cloud_batch   every tracker gets its nodes and guide nodes, its geodesic coordinate is REPLACED, its own sigma2 is left
 *                         alone; sigma2_out: NULL or F (reg's sigma2 of the frames that succeeded), rc_each: NULL or F codes. */
int tdlo_reg_batch(tdlo_ctx *ctx, const int *slots, int F, double *Y, double *sigma2, int M, double mu, int max_iter);
int tdlo_sort_pts_batch(tdlo_ctx *ctx, const double *Y, int F, int M, double *Y_sorted, int *perm, double *coord, int *rc_each);
int tdlo_tracker_initialize_from_cloud_batch(tdlo_tracker *const *trackers, int F, double mu, int max_iter, double *sigma2_out, int *rc_each);
/* Test aid, no device and no context: where the F frames of such a call keep their doubles in the workspace (csrc/tdlo_reg_plan.h).  N: the F cloud
 * sizes (>= 1).  nblk: E-step workgroups per frame, max(1, min(ceil(N / 256), 256)) as tdlo_reg's; state_off / part_off / out_off: each frame's state
 * block (8 + 3 M doubles), partial sums (nblk x (5 M + 1)) and output block (2 + 4 M + ceil(M / 2), on 16 bytes), in doubles; total: doubles in all --
 * for F = 1 what the single call asks for.  Any output may be NULL.  TDLO_E_INVALID for F < 1, M < 1, a null N or an empty cloud. */
int tdlo_debug_reg_batch_plan(const int *N, int F, int M, int *nblk, long long *state_off, long long *part_off, long long *out_off, long long *total);

/* ---- depth image -> cloud -> voxel-grid down-sample ------------------------ */
/* The step right upstream of tracking_step in the ROS node (trackdlo/src/trackdlo_node.cpp:195-241): every pixel
 * with mask != 0 is back-projected ((u - cx) z / fx, (v - cy) z / fy, z = depth / 1000; float storage like
 * pcl::PointXYZRGB, :212-232) and the points are down-sampled by pcl::VoxelGrid with a cubic leaf of `leaf_size`
 * metres (:235-239; PCL 1.10 algorithm: one centroid per occupied cell, ascending cell index; when the cell count
 * overflows int32 the cloud is passed through unchanged, as PCL does).  depth: rows x cols uint16 millimetres, mask:
 * rows x cols uint8, both row-major (cv::Mat layout).  The result becomes the cloud resident in `slot` -- what
 * tdlo_set_cloud would have uploaded (:241) -- so tdlo_cpd_lle_resident, tdlo_visibility_prepass and
 * tdlo_tracker_tracking_step (with X == NULL) run on it without the cloud ever visiting the host.
 * X_out (optional): n x 3 column-major, leading dimension n, needs x_capacity >= n rows (else TDLO_E_INVALID after
 * the cloud has been made resident); *n_out = n, *n_raw_out = number of masked pixels.  n == 0 is not an error here
 * (the registration calls report TDLO_E_INVALID for an empty cloud). */
int tdlo_depth_to_cloud(tdlo_ctx *ctx, int slot, const unsigned short *depth, const unsigned char *mask, int rows, int cols,
                        double fx, double fy, double cx, double cy, double leaf_size,
                        double *X_out, int x_capacity, int *n_out, int *n_raw_out);
/* Up to 32 704 masked pixels (a 1280 x 720 frame of the reference's camera, launch/realsense_node.launch:7-12, holds about 30 000 on the rope) the
 * whole step is ONE kernel launch (csrc/tdlo_cloud.hip: compaction, back-projection and bounding box per 4096-pixel tile; then the last eight workgroups
 * to finish sort cell index | pixel rank as a team -- k_cloud_team: they are running, hence co-resident, every wait between them is bounded and a team
 * that cannot complete hands the frame to the multi-launch form -- and form the centroids; TDLO_CLOUD_TEAM=0: the ONE workgroup that finishes last does it
 * alone in LDS, k_cloud_fused) whose last workgroup reports the counts through pinned host memory; more masked pixels, a grid whose cell-index bits + rank bits exceed 32, or PCL's pass-through case take the multi-launch
 * form (bounding box, host round trip, radix sort passes, centroids) -- the same bits either way (TDLO_CLOUD_FUSED=0 forces it; tdlo_debug_route_count
 * 6 / 7 count the calls the one-launch kernel served / passed on).  "The same bits" includes the sign of a zero: a cell's sums start from 0.0f on every route (a
 * cell whose points are all -0.0f in a coordinate gives +0.0), and PCL's pass-through ("leaf size too small") returns the masked pixels' points themselves, widened to
 * double with their bits (-0.0f stays -0.0), as step 7 of tdlo_cloud_view_voxel_grid's contract says for the view path.
 *
 * tdlo_image_buffers: pinned host buffers of the context for a rows x cols depth image and mask (valid until the next call with a larger image, or
 * tdlo_destroy).  A caller that lets its driver / segmentation write into them -- e.g. cv::Mat(rows, cols, CV_16UC1, depth) and
 * cv::Mat(rows, cols, CV_8UC1, mask) as the destinations of the conversions at trackdlo_node.cpp:167-190 -- and passes exactly these pointers
 * to tdlo_depth_to_cloud has the kernel read the images where they are, over PCIe (the mask once, coalesced; depth only where the mask is set):
 * no host-to-device copy of 3 bytes per pixel.  Any other pointers are copied to the device first, as before. */
int tdlo_image_buffers(tdlo_ctx *ctx, int rows, int cols, unsigned short **depth, unsigned char **mask);

/* ---- caller-side visibility pre-pass ----------------------------------- */
/* What the ROS node computes right before tracking_step (trackdlo/src/trackdlo_node.cpp:257-277, :345-360):
 * each node's shortest distance to the cloud resident in `slot` (M x N distances on the GPU, fp64),
 *   visible_nodes          = { m : dist_m <= visibility_threshold }, ascending          (:316, :326, :346)
 *   visible_nodes_extended = visible_nodes with occluded runs shorter than d_vis (in geodesic_coord) filled in (:350-360)
 * The OpenCV painter's-algorithm self-occlusion test (:279-343, cv::line rasterisation) is NOT part of it.
 * Points with a NaN coordinate take no part; dist_m is at most 100000, the value the reference's search starts from (:261) -- what a cloud
 * without a point at a finite distance reports.  Output arrays need room for M entries; any output pointer may be NULL. */
int tdlo_visibility_prepass(tdlo_ctx *ctx, int slot, const double *Y, int M, double visibility_threshold, double d_vis,
                            const double *geodesic_coord, double *node_dist, int *visible_nodes, int *n_vis,
                            int *visible_nodes_extended, int *n_vis_ext);

/* The same for F slots in ONE launch and one wait (k_node_min_dist_batch): slots distinct, in any order, each with a resident cloud; Y is F consecutive
 * M x 3 column-major blocks, geodesic_coord and the outputs F rows of M entries (n_vis / n_vis_ext: F entries); any output pointer may be NULL.
 * The outputs are those of F tdlo_visibility_prepass calls, bit for bit, on every route: where that call does not take its one-launch kernel
 * (TDLO_DIRECT_UPLOAD=0, M > 1024), and for F == 1 (the single call is the cheaper one: it has no frame table to fetch), this one loops over it
 * (tdlo_debug_route_count 30 / 31).  From two slots on the one launch wins: 0.038 against 0.069 ms for two, 0.054 against 1.09 ms for 32
 * (5 000 points, 45 nodes; profiles/tracker_batch_ab.txt).  A duplicate or empty slot, F < 1, F > max_frames, M < 1:
 * TDLO_E_INVALID, nothing touched. */
int tdlo_visibility_prepass_batch(tdlo_ctx *ctx, int F, const int *slots,
                                  const double *Y /* F consecutive M x 3 column-major blocks */, int M,
                                  double visibility_threshold, double d_vis,
                                  const double *geodesic_coord /* F x M */,
                                  double *node_dist /* F x M */,
                                  int *visible_nodes /* F x M */, int *n_vis /* F */,
                                  int *visible_nodes_extended /* F x M */, int *n_vis_ext /* F */);

/* One frame of the ROS node up to tracking_step in one call (trackdlo/src/trackdlo_node.cpp:195-277, :345-360): tdlo_depth_to_cloud followed by
 * tdlo_visibility_prepass of the tracker's current nodes Y against the cloud it has just made resident in `slot` -- the same outputs as the two
 * calls, bit for bit.  With up to 64 nodes and the one-launch team kernel the pre-pass rides in the SAME launch (every team member takes the minima
 * over the centroids it has just formed; the member that finishes last hands cloud size and minima to pinned host memory together): one launch and one
 * hand-over instead of two of each.  More nodes, TDLO_CLOUD_TEAM=0 / TDLO_CLOUD_FUSED=0 / TDLO_DIRECT_UPLOAD=0, more masked pixels than the one-launch
 * form takes, a team that gave its launch up: the two steps run one behind the other as before (tdlo_debug_route_count(ctx, 8) counts the frames
 * whose pre-pass rode along).  n == 0 (no masked pixel): *n_vis = *n_vis_ext = 0, no error. */
int tdlo_depth_to_cloud_visibility(tdlo_ctx *ctx, int slot, const unsigned short *depth, const unsigned char *mask, int rows, int cols,
                                   double fx, double fy, double cx, double cy, double leaf_size,
                                   const double *Y, int M, double visibility_threshold, double d_vis, const double *geodesic_coord,
                                   double *node_dist, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                   int *n_out, int *n_raw_out);

/* The ROS node's callback from the images to the nodes in one call (trackdlo/src/trackdlo_node.cpp:195-277 and :345-369): tdlo_depth_to_cloud_visibility
 * with the tracker's own nodes, visibility threshold and geodesic coordinates, then tdlo_tracker_tracking_step on the cloud left in the tracker's slot
 * (X == NULL, no H_pre).
 * NOT in this call: the callback's self-occlusion test, trackdlo_node.cpp:279-343 (edges sorted by their distance from the camera and drawn with
 * cv::line of dlo_pixel_width into an image; a node whose projected pixel lies under an edge drawn before its own is left out of visible_nodes).
 * It needs the projection matrix and OpenCV's rasteriser: BY DEFAULT it is the caller's, and for a rope that crosses itself in the image the visible
 * sets this call forms (distance threshold + gap fill only: every node within visibility_threshold of the cloud) are larger than the reference
 * callback's.  Two ways to the callback's sets: (a) the caller runs its own :279-343 (or tdlo_self_occlusion_visible + tdlo_extend_visible_nodes below) on
 * the node distances of tdlo_depth_to_cloud_visibility / tdlo_visibility_prepass and hands visible_nodes / visible_nodes_extended to
 * tdlo_tracker_tracking_step itself; (b) tdlo_tracker_set_self_occlusion(t, proj, dlo_pixel_width) -- this call then applies the library's geometric
 * restatement of the test (parity against OpenCV's rasteriser unpinned, hence off by default).
 * tests/test_cloud_gpu.py::test_a_rope_that_crosses_itself shows the default sets, both ways, and that they agree with each other.  The visible sets of the frame are returned as well (arrays of M ints, may be NULL); stats: the two tdlo_stats of
 * tracking_step.  The result is read with tdlo_tracker_get_tracking_result.  A frame whose mask selects no pixel, or none of whose nodes lies
 * within the visibility threshold of the cloud, is TDLO_E_EMPTY (the reference's callback indexes visible_nodes[size() - 1] there, :351-361);
 * the tracker's state is untouched then. */
int tdlo_tracker_frame_from_depth(tdlo_tracker *t, const unsigned short *depth, const unsigned char *mask, int rows, int cols,
                                  double fx, double fy, double cx, double cy, double leaf_size, double d_vis,
                                  int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                  int *n_out, int *n_raw_out, tdlo_stats *stats);

/* ---- down-sample clouds as they arrive: the voxel grid on cloud views ---------------------------- */
/* For a caller that holds a cloud rather than a depth image -- a PointCloud2 (organized, NaN where there is no return), a simulator's or lidar's
 * points, a tensor on the same GPU: pcl::VoxelGrid (trackdlo_node.cpp:235-241) on the view's points, on the device, into the slot's resident cloud.
 * The reference's prototype works that way (utils/tracking_test.py:452-505: organized cloud x colour mask, then the voxel down-sample).
 *
 * V(view, N, select, leaf) is the restated PCL 1.10 VoxelGrid::applyFilter of the depth path (downsample_all_data, min_points_per_voxel = 0, no filter
 * field), applied to the view's points in input order:
 *   1. Point k is ((float)x, (float)y, (float)z) of view element k.  float32 passes through unchanged; float64 is rounded to nearest-even, so a
 *      double beyond float range becomes +-inf.
 *   2. A point is kept iff all three floats are finite (PCL's !is_dense branch, always taken) and, when select != NULL, select[k] != 0.  select: N
 *      packed bytes in host or device memory (a host array is copied to the context's device mask buffer) -- an organized cloud plus the mask that
 *      tdlo_colour_mask or the caller made.
 *   3. n_raw = the number of kept points.
 *   4. n_raw == 0: TDLO_OK, *n_out = 0, and the slot is left as tdlo_depth_to_cloud leaves it for an all-zero mask (empty).
 *   5. leaf = (float)leaf_size, inv = 1.0f / leaf, a float bounding box mn, mx over the kept points;
 *        dd[d] = (long long)((mx[d] - mn[d]) * inv) + 1,  min_b[d] = (int)floorf(mn[d] * inv),  div_b[d] = (int)floorf(mx[d] * inv) - min_b[d] + 1.
 *   6. Pass-through (PCL's "leaf size too small") iff the exact product dd[0] dd[1] dd[2] exceeds 2^31 - 1.  It is evaluated without overflow: an
 *      extent term (mx[d] - mn[d]) * inv that is not finite or is >= 2^31 is pass-through outright, and the product is formed stepwise.
 *   7. Pass-through output: the KEPT points in input order, each float widened to double as it is (the sign of a zero included).  DEPARTURE FROM PCL, which copies the non-finite points as well; the prune of
 *      trackdlo.cpp:177-195 drops those anyway.
 *   8. No pass-through and a floorf(mn[d] * inv) or floorf(mx[d] * inv) outside int32: TDLO_E_INVALID, "cloud too far from the origin for this leaf
 *      size"; the slot's cloud is untouched.  DEPARTURE FROM PCL, whose cast to int is undefined there.  (So is a div_b[d] beyond int32.)
 *   9. div_b[0] div_b[1] div_b[2] >= 0xffffffff: TDLO_E_INVALID ("too many cells"), as in the depth path; the slot's cloud is untouched.
 *  10. Cell of a point p: ijk[d] = (int)(floorf(p[d] * inv) - (float)min_b[d]); key = ijk0 + ijk1 div_b0 + ijk2 div_b0 div_b1.
 *  11. One output point per occupied cell, in ascending key: float sums taken in input order, each divided by (float)count with a correctly rounded
 *      division, the result widened to double.
 *  12. The result becomes the slot's resident cloud; n, n_raw and the optional X_out are returned exactly as tdlo_depth_to_cloud returns them.
 * Consequence (the heart of tests/test_voxel_view_gpu.py): for a depth image and a mask, with P the float32 points of the masked pixels in row-major
 * order formed by the arithmetic of trackdlo_node.cpp:219-224, V(P) is bit for bit what tdlo_depth_to_cloud leaves in the slot.  Depth-born points
 * never come near the cases of 6 and 8, so the depth path's results are what they were.  tests/voxel_ref.py is the numpy statement of V.
 *
 * tdlo_voxel_grid_dims: the grid arithmetic of 5, 6 and 8 as a host helper (no context, no GPU); the depth path and the view path both go through it.
 * *nodown = 1 for pass-through (min_b = 0, div_b = 1 then).  TDLO_E_INVALID: a null pointer, (float)leaf_size not a positive finite float, a box with
 * mn > mx or a component that is not finite, the cloud-too-far case of 8. */
int tdlo_voxel_grid_dims(const float mn[3], const float mx[3], double leaf_size, int min_b[3], int div_b[3], int *nodown);
/* V on a view into `slot`.  tdlo_cloud_view_check first; location, ready_stream (which covers a device `select` too) and the staging of a host view follow
 * tdlo_set_cloud_view: a host view is packed in its own precision into the pinned staging block and the kernels read it there, a device view is read
 * in place, and no load of any width touches a byte outside tdlo_cloud_view_extent.  TDLO_E_INVALID, with the slot's cloud intact: TDLO_VIEW_ASYNC (the
 * call needs a host round trip for the box), N > 2^26 (refused before anything is allocated; the workspace is 16 N bytes), a device view that overlaps
 * the slot's resident cloud, cases 8 and 9.
 * Routes (the same bits on each; tdlo_debug_route_count 21 counts every call that reached the kernels): a view of up to 4095 x 4096 elements is first
 * handed to the ONE-LAUNCH kernel of the depth path, k_cloud_team with the view as its point source (csrc/tdlo_cloud.hip, csrc/tdlo_view_lane.h: a thread
 * takes four consecutive elements; a device `select` needs neither alignment nor padding): one launch, the counts through pinned memory, no host round
 * trip for the box.  The kernel serves up to 32 704 kept points whose cell-index bits and rank bits fit 32 (count 27) and passes everything else on
 * (count 28) -- more kept points, pass-through (6), the refusals of 8 and 9, a result that the slot's present capacity does not hold, a team that gave
 * up -- to the multi-launch form (k_cloud_bbox / k_cloud_keys / k_cloud_centroid over the view source; radix passes as for the depth path), which
 * decides those cases as before; the kernel writes nothing to the slot unless it serves the call, so a refused call finds the resident cloud intact.
 * TDLO_CLOUD_FUSED=0 or TDLO_CLOUD_TEAM=0: every view call takes the multi-launch form (the comparator; k_cloud_fused has no view instantiation). */
int tdlo_cloud_view_voxel_grid(tdlo_ctx *ctx, int slot, const tdlo_cloud_view *v, int N, const unsigned char *select, double leaf_size,
                               double *X_out, int x_capacity, int *n_out, int *n_raw_out);
/* The view counterpart of tdlo_depth_to_cloud_visibility: tdlo_cloud_view_voxel_grid into `slot` (no X_out) followed by tdlo_visibility_prepass of the
 * nodes Y against the cloud it left, the outputs of the two calls bit for bit.  With M <= 64, the one-launch kernel serving the view and
 * TDLO_DIRECT_UPLOAD on, the pre-pass rides in that launch (count 29); otherwise the two steps run one behind the other.  A view that keeps no point:
 * TDLO_OK, *n_out = *n_vis = *n_vis_ext = 0.  Refusals are those of the two calls; Y, M and geodesic_coord are checked first. */
int tdlo_cloud_view_voxel_grid_visibility(tdlo_ctx *ctx, int slot, const tdlo_cloud_view *v, int N, const unsigned char *select, double leaf_size,
                                          const double *Y, int M, double visibility_threshold, double d_vis, const double *geodesic_coord,
                                          double *node_dist, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                          int *n_out, int *n_raw_out);
/* A whole frame from a cloud view: tdlo_cloud_view_voxel_grid into the tracker's slot, tdlo_visibility_prepass with the tracker's nodes, threshold and
 * geodesic coordinates (the two through tdlo_cloud_view_voxel_grid_visibility: one launch where the one-launch kernel serves the view),
 * tdlo_tracker_tracking_step with X == NULL -- the same bits as the three calls made by hand.  The rules of
 * tdlo_tracker_frame_from_depth hold: the self-occlusion switch, TDLO_E_EMPTY (no kept point, or no visible node) with the tracker's state untouched,
 * stats.  A refused view leaves tracker and slot as they were. */
int tdlo_tracker_frame_from_cloud_view(tdlo_tracker *t, const tdlo_cloud_view *v, int N, const unsigned char *select, double leaf_size, double d_vis,
                                       int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                       int *n_out, int *n_raw_out, tdlo_stats *stats);

/* ---- colour segmentation on the device: BGR + depth frames in one call ------------------------ */
/* The callback's segmentation (trackdlo/src/trackdlo_node.cpp:158-180 with color_thresholding, :84-119): cv::cvtColor(BGR2HSV), cv::inRange over one
 * range (the launch file's hsv_threshold_*) or four (multi_color_dlo), the AND with the occlusion mask -- so that a caller hands over what the camera
 * delivers (bgr8 + 16UC1) and needs no OpenCV pass on the host.
 * The arithmetic is OpenCV's published integer routine for 8-bit images, hsv_shift = 12, hue range 180: tables sdiv[i] = rint((255 << 12) / i) and
 * hdiv[i] = rint((180 << 12) / (6 i)) (fp64, ties to even, entry 0 = 0), and per pixel in 32-bit integers
 *   v = max(b, g, r); d = v - min(b, g, r); s = (d sdiv[v] + 2048) >> 12;
 *   h = v == r ? g - b : v == g ? b - r + 2 d : r - g + 4 d;   h = (h hdiv[d] + 2048) >> 12;   h += h < 0 ? 180 : 0            (H in 0 .. 179)
 * -- not the rounded float formula (the two differ on ~2 % of the colour cube).  A pixel passes range k when lower[k][c] <= hsv[c] <= upper[k][c] on all
 * three channels; the mask is 255 where any range passes and the occluder byte (when an occluder image is given) is not 0, else 0.
 * PARITY UNPINNED against OpenCV: the routine is restated from its published algorithm (OpenCV is not part of the build image), like the painter test
 * above; tests/colour_ref.py is the numpy statement that the device code is held to bit for bit over all 2^24 colours (tests/test_colour_gpu.py).
 * Reference values (H, S, V): the launch file's range {1, {{90, 90, 30}}, {{130, 255, 255}}, 0}; color_thresholding's four:
 * {90, 90, 60} - {130, 255, 255}, {130, 60, 50} - {255, 255, 255}, {0, 60, 50} - {10, 255, 255}, {15, 100, 80} - {40, 255, 255}. */
typedef struct {
    int n_ranges;        /* 1 .. 4; anything else: TDLO_E_INVALID */
    int lower[4][3];     /* H, S, V; clamped to 0 .. 255 */
    int upper[4][3];
    int rgb_order;       /* 0: the image's bytes are B G R (the node's bgr8); 1: R G B (trackdlo/src/initialize.py:59) */
} tdlo_colour_params;
/* The segmentation on its own (one kernel, k_colour_mask: a thread takes four pixels).  colour: rows x cols x 3 uint8, occluder: rows x cols uint8 or NULL,
 * both row-major.  The mask is left in the context's device mask buffer; mask_out (rows x cols uint8) and hsv_out (rows x cols x 3 uint8: what
 * utils/color_picker.py shows, for tuning the ranges) are host buffers and may be NULL. */
int tdlo_colour_mask(tdlo_ctx *ctx, const unsigned char *colour, int rows, int cols, const tdlo_colour_params *params, const unsigned char *occluder,
                     unsigned char *mask_out, unsigned char *hsv_out);
/* Pinned host buffers of the context for a rows x cols colour image and occluder image, with the lifetime rules of tdlo_image_buffers.  A caller that
 * passes exactly these pointers (occluder: this one or NULL) to the calls below has the kernel read the images where they are, over PCIe; any other
 * pointer is copied to the device first.  (The depth image is read in place when it is tdlo_image_buffers' depth pointer.) */
int tdlo_colour_buffers(tdlo_ctx *ctx, int rows, int cols, unsigned char **colour, unsigned char **occluder);
/* tdlo_depth_to_cloud / tdlo_depth_to_cloud_visibility with the segmentation formed from the colour image instead of a mask handed in: the one-launch
 * kernels (k_cloud_team / k_cloud_fused, colour instantiation) read each thread's four pixels as 12 colour bytes + 4 occluder bytes where they read a
 * mask word, and everything behind it -- depth only where the mask is set, compaction, voxel grid, the riding pre-pass -- is the same code: the bits of
 * the mask calls fed the segmentation's mask.  Frames the one-launch kernel does not serve (more than 32 704 masked pixels, too many cell bits, PCL's
 * pass-through, a team that gave its launch up; TDLO_CLOUD_FUSED=0) take k_colour_mask and then the multi-launch form; TDLO_COLOUR_FUSED=0 (read when
 * the context is made; the comparator): k_colour_mask, then the mask route as it is.  tdlo_debug_route_count 15 / 16 count the two. */
int tdlo_colour_depth_to_cloud(tdlo_ctx *ctx, int slot, const unsigned short *depth, const unsigned char *colour, const tdlo_colour_params *params,
                               const unsigned char *occluder, int rows, int cols, double fx, double fy, double cx, double cy, double leaf_size,
                               double *X_out, int x_capacity, int *n_out, int *n_raw_out);
int tdlo_colour_depth_to_cloud_visibility(tdlo_ctx *ctx, int slot, const unsigned short *depth, const unsigned char *colour, const tdlo_colour_params *params,
                                          const unsigned char *occluder, int rows, int cols, double fx, double fy, double cx, double cy, double leaf_size,
                                          const double *Y, int M, double visibility_threshold, double d_vis, const double *geodesic_coord,
                                          double *node_dist, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                          int *n_out, int *n_raw_out);
/* tdlo_tracker_frame_from_depth from the two sensor images: the callback from the images to the nodes (trackdlo_node.cpp:158-277, :345-369) in one call.
 * The self-occlusion switch applies as it does there; a frame none of whose pixels pass is TDLO_E_EMPTY, the tracker's state untouched. */
int tdlo_tracker_frame_from_colour(tdlo_tracker *t, const unsigned short *depth, const unsigned char *colour, const tdlo_colour_params *params,
                                   const unsigned char *occluder, int rows, int cols,
                                   double fx, double fy, double cx, double cy, double leaf_size, double d_vis,
                                   int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                   int *n_out, int *n_raw_out, tdlo_stats *stats);

/* ---- clouds for many slots in one call ---------------------------------------------------------------- */
/* The front end of a batch of trackers (several ropes in a work cell, one rope seen by several cameras, many recorded sequences at once): F frames of one
 * image size become the resident clouds of F slots in one call.  An IMAGE is a set of planes of rows x cols pixels, packed and row-major as in the single
 * calls -- depth, and a mask, or a colour image (with an optional occluder image), or both; a FRAME names a slot, an image and how the image is segmented:
 * colour_params == NULL takes the image's mask, otherwise the segmentation is formed from its colour image under these ranges.  Any number of frames may
 * share an image (one camera, several ropes, each with its own ranges).  Plane pointers may be host memory or device memory of the context's GPU (the runtime
 * is asked); every distinct plane is copied once per call into the context's batch arena, device planes device to device.
 *   The frames that take a mask and the frames that take colour ranges are one launch each of k_cloud_fused_batch (grid: tiles x frames; every frame with
 * its own state words, workspace and pinned result words; no workgroup waits for another), on one stream behind the copies, followed by ONE host wait.
 * A frame the kernel does not take -- more than 32 704 masked pixels, cell-index bits + rank bits beyond 32, PCL's pass-through -- then goes through the
 * single call for its slot alone.  tdlo_debug_route_count 32 counts the frames the batch launch served, 33 the frames it passed on; 6 / 7 / 15 / 16 keep
 * counting what the single route does.
 *   BITS: every slot's cloud, n_out[f] and n_raw_out[f] are those of tdlo_depth_to_cloud / tdlo_colour_depth_to_cloud on that frame alone, the sign of a
 * zero included, whatever else shares the call and in whatever order.  A frame that selects no pixel leaves an empty cloud (n = 0), as the single call does.
 *   Refused as a whole with TDLO_E_INVALID before anything is touched (resident clouds intact): F < 1 or F greater than the context's slot count, a slot out
 * of range or named twice, an image index out of range, an image without depth or with neither mask nor colour, colour ranges on an image without colour,
 * no ranges on an image without mask, bad tdlo_colour_params, and what the single call refuses of size, leaf and intrinsics.
 *   rc_each (NULL or F codes): a frame that fails on its own (passed on, then refused by the single route) gets its code; the call returns the first one.
 *   Fewer than kCloudBatchMin frames (csrc/tdlo_api.cpp) loop over the single calls: the same bits.  MEASURED (profiles/cloud_batch_ab.txt, rope frames,
 * F = 1 .. 32): from pageable images the batch call wins from 2 frames at 640 x 480 (0.155 against 0.175 ms; 1.42 against 2.82 ms at 32) and from 3 at
 * 1280 x 720 (3.31 against 4.81 ms at 32); frames that share one image cost 0.19 ms at 32 frames of 640 x 480; but F single calls on the context's pinned
 * image buffers, read in place, beat a batch that copies caller-pinned images up at every F at 1280 x 720 (2.13 against 2.63 ms at 32) and up to 8 frames at
 * 640 x 480.  The rule "every batch value below every single-calls value at both sizes" is met by no F up to 32, so kCloudBatchMin is 33: BY DEFAULT THE
 * CALLS LOOP OVER THE SINGLE CALLS.  TDLO_CLOUD_BATCH_MIN=n (read when the context is made) turns the batch launch on from n frames -- worth it for callers
 * whose images lie in ordinary host or device memory, or who segment several ropes out of one image. */
typedef struct { const unsigned short *depth; const unsigned char *mask;      /* mask, or: */
                 const unsigned char *colour; const unsigned char *occluder;  /* colour (+ optional occluder) */
                 double fx, fy, cx, cy; } tdlo_batch_image;
typedef struct { int slot; int image; const tdlo_colour_params *colour_params; /* NULL: the image's mask */ } tdlo_batch_frame;
int tdlo_depth_to_cloud_batch(tdlo_ctx *ctx, const tdlo_batch_image *images, int K, int rows, int cols,
                              const tdlo_batch_frame *frames, int F, double leaf_size,
                              int *n_out /* F */, int *n_raw_out /* F */, int *rc_each /* F or NULL */);
/* The call above into the trackers' slots (frame i: tracker i's slot, image image_of[i], colour_params[i] or the mask), then tdlo_tracker_frame_batch on the
 * trackers whose cloud is not empty.  A tracker whose frame selects no pixel gets TDLO_E_EMPTY in rc_each and is left untouched; the others go on.  Refused as
 * tdlo_tracker_frame_batch and the call above refuse, except that no cloud need be resident.  visible_nodes / visible_nodes_extended: F rows of num_of_nodes
 * entries; stats: 2 F entries; any output may be NULL.  Bits: those of tdlo_depth_to_cloud (or its colour form) per slot + tdlo_tracker_frame_batch. */
int tdlo_tracker_frames_batch(tdlo_tracker *const *trackers, int F, const tdlo_batch_image *images, int K, int rows, int cols,
                              const int *image_of /* F */, const tdlo_colour_params *const *colour_params /* NULL or F entries, each NULL = mask */,
                              double leaf_size, double d_vis,
                              int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                              int *n_out, int *n_raw_out, tdlo_stats *stats, int *rc_each);

/* ---- one cloud from several cameras: a rig's frames fused in one launch ------------------------------------ */
/* A work cell with two or three RGB-D cameras wants ONE cloud in ONE common frame for its rope -- a node is then visible as soon as any camera sees it --
 * where the reference takes one image pair per callback (trackdlo_node.cpp:158).  A RIG is K cameras of one image size; a camera brings its depth image, a
 * mask or a colour image (with optional occluder and its own ranges), its intrinsics and, optionally, the 3 x 4 matrix that takes its frame to the common one.
 * The planes are packed and row-major as in the single calls, in host memory or in device memory of the context's GPU (the runtime is asked, as for
 * tdlo_depth_to_cloud_batch); every distinct plane is copied once per call into the context's batch arena, so that the kernels' loads stay inside memory the
 * library owns.  Depth is 16UC1 millimetres.
 *
 * THE RIG'S POINT LIST R:
 *   - for k = 0 .. K - 1 in the caller's order, the kept pixels of camera k in row-major order;
 *   - kept: mask byte != 0; in a colour rig, the segmentation of tdlo_colour_mask under that camera's ranges with its occluder byte;
 *   - the camera-frame point in double: zd = depth / 1000.0, xd = ((double)j - cx) * zd / fx, yd = ((double)i - cy) * zd / fy (pixel row i, column j) -- the
 *     arithmetic of trackdlo_node.cpp:219-224 before it is stored as float;
 *   - cam_to_rig == NULL: the point is ((float)xd, (float)yd, (float)zd), the single call's bits, the sign of a zero included;
 *   - otherwise, with cam_to_rig = [A | b]: component r is (float)(((A[r][0] * xd + A[r][1] * yd) + A[r][2] * zd) + b[r]), every product and every sum
 *     rounded to double on its own -- no fused multiply-add -- in this order;
 *   - a point whose three floats are not all finite is dropped (rule 2 of the view contract);
 *   - n_raw is the length of R.
 * The slot's cloud is V(R, leaf) of the view contract above, steps 3 - 12: pass-through, both refusals (8, 9: the slot's cloud untouched), the empty case and
 * the sign of a zero included.  Two consequences (the heart of tests/test_rig_gpu.py; tests/rig_ref.py is the numpy statement):
 *   (a) K = 1 with cam_to_rig == NULL is tdlo_depth_to_cloud (or tdlo_colour_depth_to_cloud) bit for bit;
 *   (b) for any rig, tdlo_cloud_view_voxel_grid on R held as a float32 host array leaves the same cloud bit for bit.
 * CAMERA ORDER IS PART OF THE CONTRACT: two cameras' points that share a cell are summed in float in list order.  (K calls of tdlo_depth_to_cloud and a
 * merge are something else: a voxel grid of voxel grids.)
 * A rig is segmented one way: a camera that brings a mask is segmented by it (its colour fields are not read), a camera without a mask by its colour image
 * under colour_params; all cameras of a rig the same way.  cam_to_rig need not be a rigid motion.
 * Refused as a whole with TDLO_E_INVALID before anything is touched (the resident cloud intact): K < 1 or K > 64; K rows cols > 2^26; a camera without depth;
 * a camera with neither mask nor colour; cameras that mix the two kinds; colour without ranges, or bad ranges; fx or fy equal to 0; an entry of cam_to_rig
 * that is not finite; a plane in device memory of another GPU; what the single call and V refuse of size and leaf.
 * Routes (the same bits on each): a rig of up to 4095 tiles -- K x ceil(rows cols / 4096) -- is first handed to the ONE-LAUNCH kernel, k_cloud_team with the
 * rig as its point source (csrc/tdlo_cloud.hip: tile b is camera b / Tc and fetches that camera's record of a table in device memory; csrc/tdlo_rig_point.h has
 * the lane's loads and arithmetic, shared with the host): one launch, the counts through pinned memory.  It serves up to 32 704 kept points whose cell-index bits
 * and rank bits fit 32 (tdlo_debug_route_count 45) and passes everything else on (46) -- more kept points, pass-through, the refusals of 8 and 9, a result the
 * slot's present capacity does not hold, a team that gave its launch up -- to the multi-launch form over the same element order (element p: camera p / P,
 * pixel p % P; a colour rig's masks by k_colour_mask per camera into the arena first).  TDLO_CLOUD_FUSED=0, TDLO_CLOUD_TEAM=0 or more than 4095 tiles: the
 * multi-launch form at once (counted by 46 as well: 45 + 46 are the rigs that reached the kernels).
 * MEASURED (profiles/rig_ab.txt, scripts/gpu_rig.py; rope frames, K = 1 .. 4, the clouds bit-equal on both sides): three 640 x 480 cameras cost 0.083 ms from
 * device planes and 0.182 ms from pageable host planes, against 0.83 / 0.64 ms for the composition a caller had before -- R by tdlo_rig_points_host, then
 * tdlo_cloud_view_voxel_grid -- and 1.88 / 1.68 ms with R formed by numpy; rigs the one launch passes on (more than 32 704 kept pixels: K = 4 at 640 x 480,
 * K >= 2 at 1280 x 720) take 0.6 - 1.4 ms on the multi-launch form, against 1.22 - 4.0 ms for the composition. */
typedef struct { const unsigned short *depth; const unsigned char *mask;      /* mask, or: */
                 const unsigned char *colour; const unsigned char *occluder;  /* colour (+ optional occluder) */
                 const tdlo_colour_params *colour_params;                     /* with colour: this camera's ranges */
                 double fx, fy, cx, cy;
                 const double *cam_to_rig;  /* NULL, or 12 doubles: 3 x 4 row-major [A | b], camera frame -> common frame */
               } tdlo_rig_camera;
int tdlo_rig_to_cloud(tdlo_ctx *ctx, int slot, const tdlo_rig_camera *cams, int K, int rows, int cols, double leaf_size,
                      double *X_out, int x_capacity, int *n_out, int *n_raw_out);
/* tdlo_depth_to_cloud_visibility for a rig: tdlo_rig_to_cloud into `slot` (no X_out) followed by tdlo_visibility_prepass of the nodes Y against the cloud it
 * left, the outputs of the two calls bit for bit.  With M <= 64, the one-launch kernel serving the rig and TDLO_DIRECT_UPLOAD on, the pre-pass rides in that
 * launch (tdlo_debug_route_count 47); otherwise the two steps run one behind the other.  A rig that keeps no pixel: TDLO_OK, *n_out = *n_vis = *n_vis_ext = 0. */
int tdlo_rig_to_cloud_visibility(tdlo_ctx *ctx, int slot, const tdlo_rig_camera *cams, int K, int rows, int cols, double leaf_size,
                                 const double *Y, int M, double visibility_threshold, double d_vis, const double *geodesic_coord,
                                 double *node_dist, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                 int *n_out, int *n_raw_out);
/* A whole frame from a rig: tdlo_rig_to_cloud_visibility with the tracker's own nodes, threshold and geodesic coordinates, then tdlo_tracker_tracking_step on
 * the cloud left in the tracker's slot, as tdlo_tracker_frame_from_depth composes its two -- the bits of the calls made by hand.  An empty cloud or no visible
 * node is TDLO_E_EMPTY with the tracker untouched.  A tracker whose self-occlusion switch is on (tdlo_tracker_set_self_occlusion) is refused with
 * TDLO_E_INVALID: that test is one camera's; the test for a rig is tdlo_tracker_set_rig_self_occlusion, below.  A refused rig leaves tracker and slot as they were. */
int tdlo_tracker_frame_from_rig(tdlo_tracker *t, const tdlo_rig_camera *cams, int K, int rows, int cols, double leaf_size, double d_vis,
                                int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                int *n_out, int *n_raw_out, tdlo_stats *stats);
/* The host half (csrc/tdlo_rig_host.cpp; no context, no GPU).  tdlo_rig_check: TDLO_E_INVALID for what refuses a rig call as a whole (the list above, the
 * planes' locations apart).  tdlo_rig_points_host: R of a rig whose planes lie in HOST memory, as float32 x y z per point, through the very header the kernel
 * compiles (csrc/tdlo_rig_point.h) -- to pre-compute or inspect R, and the composition (b).  Up to `capacity` points are written (R_out may be NULL:
 * count only); *n_raw_out is the length of R; TDLO_E_INVALID when R_out is too short, or the rig is refused. */
int tdlo_rig_check(const tdlo_rig_camera *cams, int K, int rows, int cols, double leaf_size);
int tdlo_rig_points_host(const tdlo_rig_camera *cams, int K, int rows, int cols, float *R_out, int capacity, int *n_raw_out);

/* ---- many ropes under one rig in one call: batched rig frames ------------------------------------------------ */
/* The cell that has two or three cameras is the cell that tracks several ropes at once: one camera set, one colour range or mask per rope.  A FRAME is a slot
 * and a rig of its own -- K_f cameras of the call's image size, each with its intrinsics, cam_to_rig and mask or colour ranges.  Frames may differ in K_f
 * (1 .. 64) and in kind (a mask rig and a colour rig may share a call; inside one frame all cameras are one kind, as in the single call).  Any number of
 * frames may name the SAME plane pointers -- F ropes under one rig, each frame with its own colour_params or mask planes --: every distinct plane (pointer and
 * kind) is copied ONCE per call into the context's rig-batch arena, a device plane device to device.
 *   BITS: for every frame the slot's cloud, n_out[f] and n_raw_out[f] are those of tdlo_rig_to_cloud on that frame alone -- R in camera order, then V(R, leaf):
 * the rig contract above stays the one statement of the result, this call adds no arithmetic of its own -- bit for bit, the sign of a zero included, whatever
 * else shares the call and in whatever order the frames stand.  A frame that keeps no pixel leaves an empty cloud (n = 0), as the single call does.  A frame
 * whose single call would end in refusal 8 or 9 of V gets that code in rc_each, its slot's cloud untouched, and the other frames complete.
 *   Refused as a whole with TDLO_E_INVALID before anything is touched (resident clouds intact): F < 1 or F greater than the context's slot count; a slot out of
 * range or named twice; any frame's rig failing tdlo_rig_check; a plane in another GPU's memory; a device plane that overlaps a batch arena.
 *   rc_each (NULL or F codes): a frame that fails on its own gets its code; the call returns the first one.
 *   Routes: the mask frames and the colour frames are one launch each of k_cloud_rig_batch (csrc/tdlo_cloud.hip: grid (most tiles of a frame, frames); block row
 * f takes frame f's descriptor out of a table in device memory -- its own K_f camera records, state words, tile regions, compacted points, tile counts and
 * pinned result words; a workgroup beyond its frame's K_f x Tc tiles leaves at once; a frame's last ticket finishes it in one workgroup; no workgroup waits
 * for another), on one stream behind the copies, followed by ONE host wait.  csrc/tdlo_rig_batch_plan.h lays the arena out and states its bytes: K times the
 * cloud batch's, about 33 MB a frame for three 1280 x 720 cameras, so one launch covers only as many frames as keep the arena within 1 GiB (kRigBatchBudget)
 * and further frames go in further launches back to back under the same wait.  A frame the kernel does not take -- more than 32 704 kept points, cell-index
 * bits + rank bits beyond 32, PCL's pass-through, a result the slot's present capacity does not hold (the slot is not grown in front of the launch: that would
 * free a cloud a refusal must leave intact) -- and a frame of more than 4095 tiles then goes through tdlo_rig_to_cloud for its slot alone; with
 * TDLO_CLOUD_FUSED=0 every frame does.  tdlo_debug_route_count 49 counts the frames the batch launch served, 50 the frames passed on; 45 - 47 keep counting what
 * the single route does.
 *   Fewer than kRigBatchMin frames (csrc/tdlo_api.cpp) loop over the single calls: the same bits.  MEASURED (profiles/rig_batch_ab.txt, scripts/gpu_rig_batch.py;
 * rope frames of 45 nodes under K = 3 cameras, F = 1 .. 32, the clouds bit-equal on both sides): at 640 x 480 the batch call loses at 1 and 2 frames and wins
 * from 4 on -- 32 ropes under one rig cost 0.70 ms against 2.18 ms from device planes and 2.05 against 6.16 ms from pageable host planes, 32 rigs with planes
 * of their own 1.04 against 2.25 ms --; at 1280 x 720 three cameras keep 96 805 pixels, the kernel passes every frame on and the call loses by 3 - 9 %.  The
 * rule "every batch value below every single-calls value at both sizes" is met by no F up to 32, so kRigBatchMin is 33: BY DEFAULT tdlo_rig_to_cloud_batch
 * LOOPS OVER THE SINGLE CALLS.  The tracker call wins on every value from 4 trackers on at both sizes (32 trackers: 2.26 against 5.69 ms at 640 x 480, 32.6
 * against 35.6 ms at 1280 x 720): kRigBatchTrackerMin is 4.  TDLO_RIG_BATCH_MIN=n (read when the context is made) sets both -- worth it for a cell whose ropes
 * keep fewer than 32 704 pixels over all cameras. */
typedef struct { int slot; const tdlo_rig_camera *cams; int K; } tdlo_rig_frame;
int tdlo_rig_to_cloud_batch(tdlo_ctx *ctx, const tdlo_rig_frame *frames, int F, int rows, int cols, double leaf_size,
                            int *n_out /* F */, int *n_raw_out /* F */, int *rc_each /* F or NULL */);
/* The call above into the trackers' slots (frames[i] is tracker i's rig; its .slot is not read), then tdlo_tracker_frame_batch on the trackers whose cloud is
 * not empty: the bits of the two calls made by hand.  A tracker whose frame keeps nothing gets TDLO_E_EMPTY in rc_each and is left untouched; the others go on.
 * A tracker with the self-occlusion switch on refuses the WHOLE call before anything is touched (the single call refuses that tracker too).  Otherwise refused
 * as tdlo_tracker_frame_batch and the call above refuse, except that no cloud need be resident.  visible_nodes / visible_nodes_extended: F rows of
 * num_of_nodes entries; stats: 2 F entries; any output may be NULL. */
int tdlo_tracker_frames_from_rig_batch(tdlo_tracker *const *trackers, int F, const tdlo_rig_frame *frames /* .slot not read */,
                                       int rows, int cols, double leaf_size, double d_vis,
                                       int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                       int *n_out, int *n_raw_out, tdlo_stats *stats /* 2 F */, int *rc_each);
/* The arena layout of csrc/tdlo_rig_batch_plan.h (no context, no GPU), shaped like tdlo_debug_view_batch_plan: frames of K[f] cameras of rows x cols pixels into
 * the slots slot[f] of a context of Fcap slots; plane: 4 keys per camera -- depth, mask, colour, occluder; 0: none --, camera after camera, frame after frame
 * (two entries with the same key and kind are one plane); budget: the bytes one launch may address (<= 0: the library's 1 GiB).  Outputs in bytes from the
 * arena's start, any may be NULL: state_off / cams_off / tiles_off / pts_off / cnt_off / launch_of: F entries; plane_off: one entry per key (-1: none).
 * Blocks of DIFFERENT launches share their place.  TDLO_E_INVALID: what the header refuses (a slot named twice, K outside 1 .. 64, more than 4095 tiles, ...).
 * tdlo_debug_rig_batch_arena: where the context's rig-batch arena lies at present (a test aid for the overlap refusal; NULL / 0 before the first batch). */
int tdlo_debug_rig_batch_plan(const int *slot, const int *K, int F, int Fcap, int rows, int cols, const unsigned long long *plane, long long budget,
                              long long *state_off, long long *cams_off, long long *plane_off, long long *tiles_off, long long *pts_off, long long *cnt_off,
                              int *launch_of, long long *table_off, long long *total, int *n_planes, int *n_launches);
int tdlo_debug_rig_batch_arena(tdlo_ctx *ctx, const void **base, long long *bytes);

/* ---- self-occlusion under a rig: a node is hidden only if every camera that sees it hides it ------------------ */
/* Where a rope crosses itself, the strand one camera sees painted over usually lies in plain view of another.  tdlo_self_occlusion_visible is one camera's test
 * (one projection matrix); THIS is the test for a rig.  Inputs: the nodes Y (M x 3 doubles, column-major as everywhere, in the rig's common frame); per camera k
 * the intrinsics fx, fy, cx, cy of cams[k] (nothing else of a tdlo_rig_camera is read) and an optional 3 x 4 row-major matrix rig_to_cam_k = [A | b] -- the
 * argument rig_to_cam is NULL (every camera frame is the rig frame) or K x 12 doubles, where a camera whose 12 entries are ALL NaN has no matrix --; the image
 * size rows x cols; dlo_pixel_width w; node_dist[M]; visibility_threshold.
 * PER CAMERA k:
 *   1. camera-frame node: x_c = ((A00 x + A01 y) + A02 z) + b0, likewise y_c, z_c -- double, every product and sum rounded on its own, left to right, never fused
 *      (the discipline of the rig's point list above); without a matrix the node as it is.
 *   2. pixel: u = fx x_c + cx z_c, v = fy y_c + cy z_c, qc = u / z_c, qr = v / z_c: tdlo_self_occlusion_visible's projection with the matrix
 *      {fx,0,cx,0, 0,fy,cy,0, 0,0,1,0}, in the same order of operations.  The node is DRAWABLE in k when z_c > 0 and both quotients lie in (-8193, 8192) (the
 *      rule of the result image; NaN and infinities fail it); its pixel is then ((int)qc, (int)qr).  It is SEEN by k when it is drawable and 0 <= c < cols,
 *      0 <= r < rows.  (The single test casts before it checks; this one checks first.)
 *   3. painted edges: edge i joins nodes i and i + 1 and is PAINTED in k when both ends are drawable; its key is sqrt(mx^2 + my^2 + mz^2) of the camera-frame
 *      mid-point ((a + b) / 2 per coordinate).  Painted edges are ranked by (key, index) ascending: nearest first, equal keys by ascending index.
 *   4. first_k(m): the smaller rank of node m's painted incident edges; the number of painted edges if it has none.
 *   5. node m is HIDDEN in k when it is drawable and some painted edge of rank < first_k(m) covers its pixel -- within w / 2 of the segment between the edge's
 *      end pixels, in exact integer arithmetic, as in the single test.
 * THE RIG'S VERDICT: node m is visible when node_dist[m] <= visibility_threshold (a NaN distance fails) AND at least one camera sees it and does not hide it.
 * A camera that does not see a node has no say: without that rule a camera looking elsewhere would vouch for every node.  The set is ascending; the extended set
 * is tdlo_extend_visible_nodes over it, as everywhere.  Camera order does not matter to the set; it does to the per-camera words.
 * CONSEQUENCE (tests/test_rig_painter_ref.py): K = 1 without a matrix and every node's pixel inside the image gives tdlo_self_occlusion_visible's set on the
 * same Y with the matrix above, the same width, distances and threshold.  Parity against OpenCV's rasteriser stays UNPINNED, as for the single test.
 * seen_words / hidden_words (optional): K x ceil(M / 32) words each, bit m % 32 of word m / 32 of camera k; in the batch call frame after frame, packed.
 *
 * tdlo_rig_self_occlusion_visible: the host statement (csrc/tdlo_painter_host.cpp through csrc/tdlo_painter_lane.h, the header the kernel compiles; no
 * context, no GPU).  tdlo_rig_self_occlusion_batch: F frames -- each its own nodes, rig, width, distances and threshold -- in ONE upload of tables and nodes,
 * ONE launch of k_rig_painter_batch (csrc/tdlo_painter.hip: grid (largest K_f, F), a workgroup is one (camera, frame) job and fetches its frame's record from a
 * table in device memory; a workgroup beyond its frame's K_f leaves at once; no workgroup waits for another), one wait; the words arrive in pinned memory and
 * the host forms union, threshold and order.  visible_nodes: F rows of Mmax entries, Mmax the largest M of the call.  Always the kernel: the same sets and
 * words as the host statement, bit for bit.
 * Both are refused as a whole with TDLO_E_INVALID before anything is touched: F < 1; M outside 1 .. 1024; K outside 1 .. 64; dlo_pixel_width outside 1 .. 255;
 * rows or cols outside 1 .. 8192; an intrinsic or a matrix entry that is not finite (a camera's 12 NaN apart); fx or fy equal to 0; a null Y, cams or node_dist.
 * tdlo_debug_route_count 51 counts the (camera, frame) jobs the kernel served, 52 the jobs the host statement did inside a tracker call.
 *
 * tdlo_tracker_set_rig_self_occlusion (K = 0: off, the default; the matrices are copied): with it on, tdlo_tracker_frame_from_rig and
 * tdlo_tracker_frames_from_rig_batch replace the pre-pass's visible set by the rig's verdict -- on the tracker's nodes as they stand before the step, with the
 * pre-pass's node_dist, the call's cameras, rows and cols --, then fill the gaps, then step.  A rig frame whose K differs from the switch's, or that the test
 * refuses, is TDLO_E_INVALID with tracker, slot and counters as they were.  The single switch (tdlo_tracker_set_self_occlusion) keeps refusing rig calls, with
 * or without this one.  Every call that is not a rig frame call ignores the switch; tdlo_tracker_render_result* draw every node after a rig frame.
 * In the batch call the kernel is enqueued in front of the batched pre-pass and its words are read after that call's wait: no wait is added.
 * Route: a tracker call with at least kRigPainterMin (camera, frame) jobs takes the kernel, below it the host statement; the same sets.  NOT MEASURED YET
 * (scripts/gpu_rig_painter.py writes profiles/rig_painter_ab.txt; the rule set beforehand: the smallest F K from which the kernel wins on every measured value
 * at M = 45 and M = 300, else a value above any batch): kRigPainterMin is above any batch, BY DEFAULT THE TRACKER CALLS RUN THE HOST STATEMENT.
 * TDLO_RIG_PAINTER_MIN=n (read when the context is made) overrides. */
typedef struct { const double *Y; int M; const tdlo_rig_camera *cams; const double *rig_to_cam; /* NULL or K x 12 */ int K; int dlo_pixel_width;
                 const double *node_dist; double visibility_threshold; } tdlo_rig_painter_frame;
int tdlo_rig_self_occlusion_visible(const double *Y, int M, const tdlo_rig_camera *cams, const double *rig_to_cam, int K, int rows, int cols,
                                    int dlo_pixel_width, const double *node_dist, double visibility_threshold,
                                    int *visible_nodes, int *n_vis, unsigned *seen_words /* NULL or K x ceil(M / 32) */, unsigned *hidden_words);
int tdlo_rig_self_occlusion_batch(tdlo_ctx *ctx, int F, const tdlo_rig_painter_frame *frames, int rows, int cols,
                                  int *visible_nodes /* F x Mmax */, int *n_vis /* F */, unsigned *seen_words, unsigned *hidden_words);
int tdlo_tracker_set_rig_self_occlusion(tdlo_tracker *t, const double *rig_to_cam /* NULL or K x 12 */, int K, int dlo_pixel_width);

/* ---- ropes that hide one another: the painter test over a cell of ropes ----------------------------------------- */
/* Every test above looks at ONE rope's own edges.  In a harness of cables rope A lying over rope B is the normal case: B's nodes under the crossing stay
 * "visible", the shared-cloud split gives the crossing's points to whichever rope has the nearer node, and B is pulled towards A's points.  THIS is the painter
 * test with every rope of the cell painted into the same picture.
 * A CELL: F ropes in the caller's order, rope f with nodes Y_f (M_f x 3 doubles, column-major), node_dist_f[M_f] and visibility_threshold_f; ONE rig (cams,
 * rig_to_cam NULL or K x 12, K, rows, cols, exactly as in "self-occlusion under a rig") and ONE dlo_pixel_width w.  The FLAT INDEX of node m of rope f is
 * n = off_f + m with off_f = M_0 + ... + M_{f-1}; N = sum of the M_f is the number of nodes of the cell.
 * PER CAMERA k:
 *   1. Steps 1 and 2 of "self-occlusion under a rig", word for word, for every node of every rope: the camera-frame node without fused multiply-adds, the
 *      pixel, DRAWABLE and SEEN.
 *   2. edges: edge (f, i) joins nodes i and i + 1 of rope f and has the flat index off_f + i.  NO edge joins the last node of one rope to the first node of the
 *      next.  An edge is PAINTED when both of its ends are drawable; its key is that section's key of its camera-frame ends.
 *   3. order: all painted edges of the cell are ordered together by (key, flat edge index) ascending.
 *   4. first_k(n): the earlier, in that order, of node n's painted incident edges (edges of its own rope only).  A node without a painted incident edge stands
 *      after every painted edge -- the only node of a rope with M_f = 1 among them.
 *   5. node n is HIDDEN in k when it is drawable and some painted edge of ANY rope covers its pixel (within w / 2 of the segment between the edge's end pixels,
 *      in exact integer arithmetic, unchanged) and stands STRICTLY before first_k(n).
 * THE VERDICT: node (f, m) is visible when node_dist_f[m] <= visibility_threshold_f (a NaN distance fails) AND at least one camera sees it and does not hide
 * it.  A camera that does not see a node has no say.  The sets are per rope, ascending, in rope-local indices.
 * CONSEQUENCES (tests/test_cell_painter_ref.py): (a) F = 1 gives the set and the words of tdlo_rig_self_occlusion_visible, bit for bit.  (b) The ropes of a
 * cell may be permuted: that changes a verdict only through the tie rule of equal keys (the flat index decides).  Parity against OpenCV's rasteriser stays
 * UNPINNED, as everywhere.
 * seen_words / hidden_words (optional): K x ceil(N / 32) words a cell, bit n % 32 of word n / 32 of camera k, n the flat index; in the batch call each of the two
 * arrays holds its words cell after cell, packed.
 * "Ordered" is the statement's wording: an implementation may decide "before" by comparing (key, flat index) pairs and never sort; this one does.
 *
 * tdlo_cell_occlusion_visible: the host statement (csrc/tdlo_cell_painter_host.cpp through csrc/tdlo_cell_painter_lane.h, the header the kernels compile;
 * no context, no GPU).  visible_nodes: F pointers, rope f's to M_f entries; n_vis: F counts.
 * tdlo_cell_occlusion_batch: C cells of one image size -- each its own ropes, rig and width -- in ONE upload, TWO launches and ONE wait
 * (csrc/tdlo_cell_painter.hip).  Per camera the work is N nodes x N edges, so one workgroup per (camera, cell) would leave the device idle: a job is spread
 * over node blocks, grid (node blocks of 256 of the largest cell, largest K, cells), lane = flat node; a workgroup beyond its cell's node count or its cell's K
 * leaves at once; nobody waits for anybody, there is no grid barrier.  k_cell_project writes the (camera, cell) table of 16-byte records (key of the edge that
 * starts at the node, the pixel as two int16, flags) and the seen words; k_cell_cover keeps its node's pixel and threshold pair (key, flat index of first_k(n))
 * in registers, streams the cell's table through LDS in tiles of 512 edges (every lane reads the same record: a broadcast), tests per edge painted, "before my
 * threshold", a pixel box reject, then the exact coverage, and stops testing as soon as no drawable node of the wave is undecided.  The words arrive in pinned
 * host memory (ballots, stored by lane 0); the host forms union, thresholds and sets.  visible_nodes: sum over the cells of F_c rows of Mmax entries, Mmax the
 * largest M_f of the call, cell after cell in rope order; n_vis likewise.  Always the kernels: the host statement's sets and words, bit for bit.
 * REFUSED as a whole with TDLO_E_INVALID, nothing touched: every refusal of the rig test (K outside 1 .. 64; dlo_pixel_width outside 1 .. 255; rows or cols
 * outside 1 .. 8192; an intrinsic or matrix entry that is not finite, a camera's 12 NaN apart; fx or fy 0; a null Y, cams or node_dist); F < 1; M_f outside
 * 1 .. 1024; N > 16 384 (kCellPainterMaxNodes: every node meets every edge and a call's time on shared hardware must stay bounded, as for the cluster call);
 * in the batch call fewer than 1 or more than 1024 cells.
 *
 * tdlo_tracker_frames_from_shared_cloud_occluded_batch: tdlo_tracker_frames_from_shared_cloud_batch with the cell's verdict in place of every tracker's
 * visible set.  (1) the split and the pre-pass as there; (2) the F trackers' ropes, in the call's order, are ONE cell under `view`; every tracker's visible
 * set is the cell's verdict on its rope -- formed on the trackers' nodes as they stand before the step, with the pre-pass's node_dist and the tracker's own
 * threshold; (3) the gap fill (tdlo_extend_visible_nodes); (4) tdlo_tracker_tracking_step_batch.  It is the composition tdlo_cloud_assign_visibility,
 * tdlo_cell_occlusion_visible, tdlo_extend_visible_nodes, tdlo_tracker_tracking_step_batch made by hand, bit for bit.  A tracker with either self-occlusion
 * switch on (tdlo_tracker_set_self_occlusion, tdlo_tracker_set_rig_self_occlusion) is refused with TDLO_E_INVALID and nothing is touched: the cell test
 * subsumes both.  So is what the cell test refuses (F M > 16 384 among it).  A tracker that owns no point gets TDLO_E_EMPTY and stays untouched, as in the
 * existing call; its rope still takes part in the cell as an occluder.  On the kernel route the two launches are enqueued in front of the split, whose wait
 * they share: the call adds no host wait (the pre-pass's distances are needed on the host alone, for the threshold; nothing on the device depends on them).
 * ROUTE RULE (set before anything was measured): the tracker call takes the kernels from kCellPainterMin (flat nodes x cameras, N K) on and the host
 * statement below it; kCellPainterMin is the smallest measured N K at and above which the kernels are faster on every measured line of
 * profiles/cell_painter_ab.txt (scripts/gpu_cell_painter.py: F = 2, 4, 8, 32 ropes of 45 nodes and 16 ropes of 1024 nodes, each at K = 1 and K = 3), a value
 * above any cell if they win nowhere.  MEASURED (one cell, kernels against host statement, ms, every compared pair bit-equal): N K = 90: 0.053 / 0.012; 180:
 * 0.079 / 0.029; 270: 0.053 / 0.025; 360: 0.139 / 0.122; 540: 0.082 / 0.095; 1080: 0.137 / 0.446; 1440: 0.454 / 2.01; 4320: 0.458 / 5.39; 16 384 (16 ropes of
 * 1024 nodes, K = 1): 4.16 / 180.5; 49 152 (K = 3): 4.19 / 540.2.  kCellPainterMin = 540.  The tracker call (F ropes of 45 nodes, 750 F points, kernels / host
 * statement / tdlo_tracker_frames_from_shared_cloud_batch without the test): F = 2: 0.29 / 0.26 / 0.25 at K = 1, 0.29 / 0.28 / 0.25 at K = 3; F = 4: 0.37 /
 * 0.33 / 0.30 and 0.37 / 0.41 / 0.30; F = 8: 0.61 / 0.62 / 0.49 and 0.62 / 0.83 / 0.50; F = 32: 3.28 / 4.31 / 1.32 and 3.67 / 7.64 / 1.28 (the trackers of
 * the two sides of the last comparison do not see the same visible sets, so they do not run the same registrations).
 * TDLO_CELL_PAINTER_MIN=n (n >= 0, read when the context is made) overrides; 0: always the kernels.  Both routes give the same bits.
 * Route counters 57 / 58: (camera, cell) jobs the kernels served / jobs the host statement did inside the tracker call.
 * OUT OF SCOPE: a joint E-step over all ropes' nodes; parity against OpenCV's rasteriser. */
typedef struct { const double *Y; int M; const double *node_dist; double visibility_threshold; } tdlo_cell_rope;
typedef struct { const tdlo_cell_rope *ropes; int F; const tdlo_rig_camera *cams; const double *rig_to_cam; /* NULL or K x 12 */ int K; int dlo_pixel_width; } tdlo_cell;
typedef struct { const tdlo_rig_camera *cams; const double *rig_to_cam; /* NULL or K x 12 */ int K; int rows, cols; int dlo_pixel_width; } tdlo_cell_view;
int tdlo_cell_occlusion_visible(const tdlo_cell_rope *ropes, int F, const tdlo_rig_camera *cams, const double *rig_to_cam, int K, int rows, int cols,
                                int dlo_pixel_width, int *const *visible_nodes /* F rows of M_f */, int *n_vis /* F */,
                                unsigned *seen_words /* NULL or K x ceil(N / 32) */, unsigned *hidden_words);
int tdlo_cell_occlusion_batch(tdlo_ctx *ctx, int C, const tdlo_cell *cells, int rows, int cols,
                              int *visible_nodes /* (sum F_c) x Mmax */, int *n_vis /* sum F_c */, unsigned *seen_words, unsigned *hidden_words);
int tdlo_tracker_frames_from_shared_cloud_occluded_batch(tdlo_tracker *const *trackers, int F, int src_slot, double d_max, double d_vis,
                                                         const tdlo_cell_view *view, int *visible_nodes /* F x M or NULL */, int *n_vis,
                                                         int *visible_nodes_extended, int *n_vis_ext, int *n_each /* F or NULL */, tdlo_stats *stats, int *rc_each);

/* ---- ropes of one colour: one cloud dealt out among F trackers on the device ------------------------------------ */
/* Every entrance above gives each rope a cloud of its own -- its own mask, its own colour ranges.  A harness of identical cables has ropes no segmentation
 * can tell apart: ONE cloud and F trackers.  These calls deal one resident cloud out among F slots on the device and step the trackers on it.
 * THE STATEMENT.  X: the n points resident in src_slot, as tdlo_get_cloud returns them.  Rope f = 0 .. F - 1: nodes Y_f (M_f x 3 column-major, all finite).
 *   D(i, f)      = min over m of node_point_d2(Y_f[m], X_i) -- the pre-pass's own distance, same argument order, same fused form:
 *                  fma(dz, dz, fma(dy, dy, fl(dx dx))) with dx = fl(y - x); the minimum is fmin (a NaN never wins); +inf if every term is NaN
 *   g(i)         = min over f of D(i, f)
 *   owner(i)     = the LOWEST f with D(i, f) = g(i) if g(i) is finite and g(i) <= fl(d_max d_max); otherwise -1 (a point with a NaN or infinite coordinate
 *                  is never owned).  d_max = INFINITY: no gate; d_max <= 0 or NaN: TDLO_E_INVALID
 *   owner_d2(i)  = g(i)
 * RESULT.  Slot ropes[f].slot becomes the cloud of the points with owner(i) = f, in ascending i, every coordinate copied bit for bit (the sign of a zero
 * counts), and is left exactly as tdlo_set_cloud of those points leaves it (the slot's sorted cloud no longer serves; an LLE regulariser left behind by a
 * tracker stays, as it does there).  A rope that owns nothing leaves a cloud of 0 points, as tdlo_rig_to_cloud leaves a slot whose rig kept no pixel.
 * n_each[f] and n_unowned (the points with owner -1) are returned; owner / owner_d2 (n entries each, or NULL) cost a copy and a wait of their own.
 * Nearest NODE, not nearest segment: it is the pre-pass's own distance, the one every pre-pass kernel shares, and it has one right bit pattern; at the node
 * spacing trackers run at (a centimetre or two) a point's distance to the chain and to its nearest node differ by less than any useful gate.
 * tdlo_cloud_assign_host is the same statement on the host (the lane of csrc/tdlo_assign_lane.h point by point; no HIP, no context; .slot is not read).
 * tdlo_cloud_assign_visibility: the outputs of tdlo_cloud_assign followed by tdlo_visibility_prepass on each destination slot, bit for bit (a node's minimum
 * over the points its rope owns does not depend on how points are dealt to lanes; sqrt, the cap of 100000, the <= test and the gap fill are that call's host
 * code).  Per-rope outputs are F pointers (rope f's: M_f entries), n_vis / n_vis_ext F counts; any output may be NULL.  A rope that owns nothing reports
 * 100000 everywhere and n_vis = 0.
 * tdlo_tracker_frames_from_shared_cloud_batch: the split by the trackers' CURRENT nodes into the trackers' own slots, the self-occlusion switch of a tracker
 * applied as tdlo_tracker_frame_batch applies it, then tdlo_tracker_tracking_step_batch: the bits of tdlo_cloud_assign + tdlo_tracker_frame_batch made by hand.
 * A tracker that owns no point, or has no visible node, gets TDLO_E_EMPTY in rc_each and is untouched; the others go on.  Refusals: tdlo_tracker_frame_batch's
 * (except that the slots need no cloud beforehand) and those below.
 * REFUSED as a whole with TDLO_E_INVALID, every destination cloud, tracker and route counter untouched: src_slot among the destinations; duplicate
 * destinations; a source or destination slot the context does not have; F < 1 or F > max_frames; M_f < 1; a node that is not finite; a bad d_max.  A source of
 * 0 points is TDLO_OK with every count 0 and every destination empty (the library does not tell a slot nobody filled from a cloud of 0 points: both are what
 * tdlo_get_cloud reports as n = 0).
 * KERNELS (csrc/tdlo_assign.hip): k_assign_count -- lane = point, the flat node list staged through LDS in tiles of 512 nodes, the running (g, owner) in
 * registers, ropes in ascending order and `<` replaces; owner and g per point, an F-vector of counts per workgroup from one wave ballot per rope present --
 * and k_assign_scatter -- every workgroup forms its F offsets from the preceding workgroups' counts (nobody waits for anybody), ranks its points by rope
 * (ballot + popcount below the lane, the waves' counts in LDS) and writes x, y, z at column stride n_f; the workgroup that draws the last ticket hands the
 * counts to pinned host memory and raises the word the host waits on.  Two launches and ONE host wait per call; every destination is sized for n beforehand
 * (its capacity grows as tdlo_set_cloud grows it).  THE RIDE: in k_assign_scatter, per rope present in a wave, that rope's nodes against the wave's points
 * (d2 = owner == f ? node_point_d2 : +inf, the wave's minimum, one atomic minimum on the ordered bits per (wave, node), as k_node_min_dist_batch does); the
 * minima go to the host with the counts, so the pre-pass costs no launch and no wait of its own.
 * ROUTE RULE (set before measuring): the ride stays the default of the tracker call and of tdlo_cloud_assign_visibility only if it is no slower than
 * tdlo_cloud_assign + tdlo_visibility_prepass_batch on every measured line of profiles/cloud_assign_ab.txt (scripts/gpu_cloud_assign.py).  MEASURED (F = 2, 4, 8, 32 ropes of 45 nodes,
 * 5 000 F points, tdlo_cloud_assign_visibility, bit-equal pairs): ride on 0.142 / 0.259 / 0.536 / 2.198 ms against ride off 0.110 / 0.190 / 0.353 / 1.398 ms --
 * slower on every line (every wave of an interleaved cloud meets every rope, and the per-slot pre-pass reads only its own points).
 * THE RIDE IS OFF BY DEFAULT, TDLO_ASSIGN_RIDE=1 (read when the context is made) turns it on.  Both routes give the same bits.  A rope of more than 1024
 * nodes, or TDLO_DIRECT_UPLOAD=0 (the pre-pass's own fall-back), takes the two calls.
 * Route counters 53 / 54: calls the split launches served (a source of 0 points launches nothing and is not counted) / calls in which the pre-pass rode.
 * OUT OF SCOPE: a joint E-step over all ropes' nodes.  (One rope hiding another: "ropes that hide one another" above,
 * tdlo_tracker_frames_from_shared_cloud_occluded_batch.  Starting F same-coloured ropes from one cloud: the next section.) */
typedef struct { int slot; const double *Y; int M; } tdlo_assign_rope;
int tdlo_cloud_assign(tdlo_ctx *ctx, int src_slot, const tdlo_assign_rope *ropes, int F, double d_max,
                      int *n_each /* F or NULL */, int *n_unowned, int *owner /* n or NULL */, double *owner_d2 /* n or NULL */);
int tdlo_cloud_assign_visibility(tdlo_ctx *ctx, int src_slot, const tdlo_assign_rope *ropes, int F, double d_max,
                                 double visibility_threshold, double d_vis, const double *const *geodesic_coord /* F rows of M_f */,
                                 int *n_each, int *n_unowned, double *const *node_dist, int *const *visible_nodes, int *n_vis,
                                 int *const *visible_nodes_extended, int *n_vis_ext);
int tdlo_cloud_assign_host(const double *X, int n, const tdlo_assign_rope *ropes /* .slot not read */, int F, double d_max,
                           int *owner, double *owner_d2, int *n_each, int *n_unowned);
int tdlo_tracker_frames_from_shared_cloud_batch(tdlo_tracker *const *trackers, int F, int src_slot, double d_max, double d_vis,
                                                int *visible_nodes /* F x M or NULL */, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                                int *n_each /* F or NULL */, tdlo_stats *stats, int *rc_each);

/* ---- starting ropes of one colour: one cloud clustered into F trackers on the device ---------------------------- */
/* The calls above need trackers that are already started.  These START them: the one cloud of F same-coloured ropes is clustered on the device (Euclidean
 * cluster extraction, as PCL users know it), cluster c becomes the cloud of destination c, and tdlo_tracker_initialize_from_cloud_batch starts the trackers.
 * THE STATEMENT.  X: the n points resident in src_slot, as tdlo_get_cloud returns them.
 *   finite       point i is finite if x, y and z are all finite; a point that is not takes part in nothing
 *   link(i, j)   i != j, both finite, and node_point_d2(X_i, X_j) <= fl(tol tol) -- the pre-pass's own distance in the fused form tdlo_cloud_assign uses:
 *                fma(dz, dz, fma(dy, dy, fl(dx dx))) with dx = fl(a - b); symmetric in its arguments (the differences negate exactly).
 *                tol <= 0, NaN or infinite: TDLO_E_INVALID
 *   clusters     the connected components of the link graph over the finite points (single linkage); root(i) = the smallest index in i's component,
 *                size(r) = its member count; a cluster is KEPT if size >= min_size.  min_size < 1: TDLO_E_INVALID
 *   numbering    the kept clusters are numbered c = 0 .. C - 1 in ascending order of their root: the order of first appearance in the cloud.  NOT PCL's order
 *                by size: it must not depend on scheduling, and ties in size are common
 *   owner(i)     with F destinations: the number of i's cluster if the cluster is kept and its number is < F; otherwise -1 (a point that is not finite, a
 *                point of a cluster that is too small, a point of a kept cluster numbered >= F)
 * RESULT.  Destination dst_slots[f] becomes the cloud of the points with owner(i) = f, in ascending i, every coordinate copied bit for bit, and is left exactly as
 * tdlo_set_cloud of those points leaves it: tdlo_cloud_assign's RESULT paragraph applies word for word.  A destination f >= C is left with 0 points.  Returned:
 * n_clusters = C (it may exceed F), n_each[F], n_unowned (the points with owner -1); owner (n entries, or NULL) costs a copy and a wait of its own.
 * tdlo_cloud_cluster_host is the same statement on the host, in the plain all-pairs form (the lane of csrc/tdlo_cluster_lane.h, every point against every
 * point in front of it; no HIP, no context): it is the statement, not a competitor.
 * tdlo_tracker_initialize_from_shared_cloud_batch: tdlo_cloud_cluster into the trackers' OWN slots, then -- C = F -- tdlo_tracker_initialize_from_cloud_batch on
 * them: that composition's bits, cluster c to trackers[c].  C != F: TDLO_E_INVALID with n_clusters and n_each written and every tracker untouched (rc_each is not
 * written); THE SLOTS HOLD THE SPLIT.  Refused as a whole, slots included: the refusals below with the trackers' slots as destinations; a null tracker; trackers of
 * different contexts or node counts; fewer than 4 nodes or more than tdlo_reg fits; max_iter < 0; mu outside [0, 1).
 * REFUSED as a whole with TDLO_E_INVALID, every destination cloud, tracker and route counter untouched: src_slot among the destinations; duplicate destinations;
 * a source or destination slot the context does not have; F < 1 or F > max_frames; a bad tol or min_size; n > 262 144 -- the device route tests ALL pairs and on
 * shared hardware a call's time must stay bounded (kClusterMaxPoints, csrc/tdlo_cluster_lane.h; the host call refuses the same n).  A source of 0 points is
 * TDLO_OK with every count 0 and every destination empty.
 * KERNELS (csrc/tdlo_cluster.hip).  The forest is one int per point, parent[i] <= i, and a word only ever decreases.  k_cluster_link -- lane = point i, the cloud
 * staged through LDS in tiles of 512 points, a workgroup per (256 points, tile) and only the tiles at or below the lane's own, every point j < i within the gate
 * joined to i's tree (the links of 64 points gathered as a word of bits, their parents loaded four at a time; a point that hangs under the lane's root already is
 * skipped): the larger root is hooked under the smaller by an agent-scope compare-and-swap, find shortens its path by an atomic minimum.  Nobody waits for anybody (no grid barrier, no
 * spinning on another workgroup, no residency assumption); every walk descends strictly and every retry follows a hook somebody else made, so the loops end, and
 * the root of a component is its smallest index WHATEVER the schedule: one right bit pattern.  The retry loop is bounded all the same (1024 attempts); a lane
 * that runs out raises a word in pinned memory and the driver serves the call by the host route -- never a wrong split.  Then k_cluster_flatten (root per point,
 * one atomic add per finite point for the sizes), k_cluster_count / k_cluster_rank (kept roots per workgroup; every workgroup sums the counts in front of it
 * itself), k_cluster_owner (owner per point and the per-workgroup counts in k_assign_count's layout) and tdlo_cloud_assign's own k_assign_scatter, unchanged:
 * the stable scatter, the counts to pinned memory, the word the host waits on.  ONE host wait per call; the workspace (3 n ints) grows with the split's buffers.
 * ROUTES.  TDLO_CLUSTER=host (read when the context is made): tdlo_get_cloud's copy, tdlo_cloud_cluster_host's owners, their per-workgroup counts formed on the
 * host, one copy up, the same k_assign_scatter.  Both routes give the same bits.  ROUTE RULE (set before measuring): the device route is the default unless it is
 * slower than the host route on every measured line of profiles/cloud_cluster_ab.txt (scripts/gpu_cloud_cluster.py).  MEASURED (F = 2, 4, 8, 32 ropes of 45
 * nodes, 5 000 F points, tol = 24 mm, bit-equal pairs): tdlo_cloud_cluster 0.95 / 2.74 / 3.00 / 9.24 ms on the device route against 151 / 556 / 2 143 / 32 832 ms
 * on the host route (the all-pairs statement: the ratio flatters the device) -- faster on every line: THE DEVICE ROUTE IS THE DEFAULT.  What clustering adds to
 * tdlo_tracker_initialize_from_cloud_batch on clouds split beforehand: 1.0 / 2.6 / 3.0 / 9.2 ms.
 * Route counters 55 / 56: calls served by the cluster launches / by the host route (forced, or after a give-up); a source of 0 points launches nothing and counts
 * in neither.
 * OUT OF SCOPE: separating ropes that TOUCH in the first frame (single linkage makes them one cluster: C < F and the tracker call refuses); choosing F from the
 * cloud; a spatial grid in place of the all-pairs pass; max_size. */
int tdlo_cloud_cluster(tdlo_ctx *ctx, int src_slot, const int *dst_slots /* F */, int F, double tol, int min_size,
                       int *n_clusters, int *n_each /* F or NULL */, int *n_unowned, int *owner /* n or NULL */);
int tdlo_cloud_cluster_host(const double *X, int n, int F, double tol, int min_size, int *owner, int *n_clusters, int *n_each, int *n_unowned);
int tdlo_tracker_initialize_from_shared_cloud_batch(tdlo_tracker *const *trackers, int F, int src_slot, double tol, int min_size, double mu, int max_iter,
                                                    double *sigma2_out /* F or NULL */, int *n_clusters, int *n_each /* F or NULL */, int *rc_each);

/* ---- cloud views for many slots in one call ----------------------------------------------------------- */
/* The same front end for callers who come with CLOUDS (the reference's own input, trackdlo_node.cpp:242; a PointCloud2; torch tensors on the device): F cloud
 * views become the resident clouds of F slots in one call -- down-sampled (tdlo_cloud_view_voxel_grid_batch) or as they are (tdlo_set_cloud_view_batch).
 * A FRAME names a slot, a view, its N and optional selection bytes (NULL: every element).  Frames may differ in N, dtype, strides, location and
 * ready_stream; any number of frames may name the SAME view with different selection bytes (one organized cloud, several ropes).
 *   tdlo_cloud_view_voxel_grid_batch: per frame the result is exactly tdlo_cloud_view_voxel_grid(ctx, slot, view, N, select, leaf_size, NULL, 0, ...) on that
 * frame alone -- V above, rules 1 - 12, the sign of a zero included -- whatever else shares the call and in whatever order; a frame that keeps no point leaves
 * an empty cloud (n = 0).  ONE launch of k_cloud_view_batch (csrc/tdlo_cloud.hip; grid: tiles of the largest frame x frames; the frame's load form -- float64,
 * 12-byte points, column-major pairs, element by element -- behind a workgroup-uniform switch in front of phase A; every frame with its own state words,
 * tile regions, compacted points, tile counts and pinned result words; no workgroup waits for another: a workgroup beyond its frame's tiles leaves at once,
 * the last ticket of a frame finishes it) and ONE host wait.  Device views are read in place (one event per distinct ready_stream); host views are packed
 * column-major in their own precision into one pinned block, a view named by several frames once, and read there by the kernel, as the single call does;
 * host selection bytes are copied into the same block and read in place as well (the kernel reads each byte once: a copy to the device would move the same
 * bytes over the same link behind one more command on the stream).  The arena's layout is csrc/tdlo_view_batch_plan.h (tdlo_debug_view_batch_plan).
 *   A frame goes into the launch when TDLO_CLOUD_FUSED is on and its N <= 1 048 576 (256 tiles); the kernel passes on what the one-launch form passes on --
 * more than 32 704 kept points, cell-index bits + rank bits beyond 32, pass-through, the cases 8 / 9.  Every other frame, and every frame passed on, goes
 * through the single call for its slot alone, which decides those cases as before; its code goes to rc_each, and the call returns the first non-zero code.
 * tdlo_debug_route_count 38 counts the frames the batch launch served, 39 the frames passed on; 21 / 27 / 28 keep counting what the single route does.
 *   Refused as a whole with TDLO_E_INVALID before anything is touched (resident clouds intact): F < 1 or F greater than the context's slot count, a slot out of
 * range or named twice, a view tdlo_cloud_view_check refuses, TDLO_VIEW_ASYNC on any view, N > 2^26, a leaf that is not a positive finite float, a pointer
 * on another GPU, a device view (or device select) that overlaps the resident cloud of ANY slot the call names.  Past that point the named slots' former
 * clouds are gone, as for tdlo_depth_to_cloud_batch.
 *   tdlo_set_cloud_view_batch: per slot what tdlo_set_cloud_view leaves, bit for bit, by ONE launch of k_cloud_import_batch (csrc/tdlo_import.hip: grid
 * (blocks of the largest frame, F), the single kernel's loaders behind a switch on the frame's form; no load touches a byte outside a view's extent) and one
 * wait.  Host views are packed into the pinned block and read in place (TDLO_VIEW_INPLACE=0: copied to the device first).  Refusals as above (no leaf, no
 * select); TDLO_VIEW_ASYNC is refused here too.  tdlo_debug_route_count 40 counts the frames the batch launch imported, 41 the frames of calls below
 * the crossover, which take the single route.
 *   CROSSOVERS (csrc/tdlo_api.cpp; below them the calls loop over the single calls: the same bits).  MEASURED (profiles/view_batch_ab.txt, _run2.txt, rope
 * clouds of 5 000 points and organized 640 x 480 clouds, F = 1 .. 32, batch and single calls alternating): one frame costs more as a batch (voxel grid 0.058
 * against 0.041 ms, import 0.021 against 0.014 ms); from 2 frames on every value of every voxel and import line wins -- 4 device views 0.058 against 0.163 ms,
 * 32 device views 0.063 against 1.29 ms, 32 host views at PointXYZRGB's stride 0.19 against 1.45 ms, 32 organized clouds under selections 0.17 against 1.19 ms
 * (one cloud shared by 32 frames: 0.16 against 1.19), the import 0.024 against 0.43 ms (device) and 0.15 against 0.56 ms (host);
 * tdlo_tracker_frames_from_cloud_view_batch 1.92 against 5.27 ms for 32 trackers, but with the registrations' own spread it won on every value from 4 trackers
 * on in one run and from 8 in others.  The rule set beforehand -- the smallest F from which every batch value lies below every single-calls value -- over the
 * lines a call stands for gives TWO constants: kViewBatchMin = 2 for tdlo_cloud_view_voxel_grid_batch and tdlo_set_cloud_view_batch called by themselves,
 * kViewBatchTrackerMin = 8 for the two tracker calls below (tdlo_tracker_tracking_step_view_batch has no line of its own and takes the same).
 * TDLO_VIEW_BATCH_MIN=n (read when the context is made) overrides both. */
typedef struct { int slot; const tdlo_cloud_view *view; int N; const unsigned char *select; /* NULL: every element */ } tdlo_view_frame;
int tdlo_cloud_view_voxel_grid_batch(tdlo_ctx *ctx, const tdlo_view_frame *frames, int F, double leaf_size,
                                     int *n_out /* F */, int *n_raw_out /* F */, int *rc_each /* F or NULL */);
int tdlo_set_cloud_view_batch(tdlo_ctx *ctx, const int *slots, const tdlo_cloud_view *const *views, const int *N, int F, int *rc_each /* F or NULL */);
/* tdlo_set_cloud_view_batch into the trackers' slots, enqueued without a host wait (device sources must stay valid until the call returns), then
 * tdlo_tracker_tracking_step_batch: the bits and the refusals of the two, except that no cloud need be resident. */
int tdlo_tracker_tracking_step_view_batch(tdlo_tracker *const *trackers, int F, const tdlo_cloud_view *const *views, const int *N,
                                          const int *const *visible_nodes, const int *n_vis, const int *const *visible_nodes_extended, const int *n_vis_ext,
                                          const double *const *H_pre, tdlo_stats *stats, int *rc_each);
/* tdlo_cloud_view_voxel_grid_batch into the trackers' slots (frame i: tracker i's slot -- the slot of the record is ignored), then tdlo_tracker_frame_batch on
 * the trackers whose cloud is not empty.  A tracker whose view keeps no point gets TDLO_E_EMPTY in rc_each and is left untouched; the others go on.  Outputs
 * as for tdlo_tracker_frames_batch; the bits and the refusals are those of the parts, except that no cloud need be resident. */
int tdlo_tracker_frames_from_cloud_view_batch(tdlo_tracker *const *trackers, int F, const tdlo_view_frame *frames /* slot ignored: the tracker's */,
                                              double leaf_size, double d_vis,
                                              int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                              int *n_out, int *n_raw_out, tdlo_stats *stats, int *rc_each);
/* Test aid: where tdlo_cloud_view_voxel_grid_batch keeps the blocks of F frames of N[f] elements in its arena (csrc/tdlo_view_batch_plan.h; offsets in bytes;
 * any output may be NULL; Fcap: the context's slot count).  TDLO_E_INVALID for F < 1, F > Fcap or an N[f] outside 1 .. 1 048 576. */
int tdlo_debug_view_batch_plan(const int *N, int F, int Fcap, long long *state_off, long long *tiles_off, long long *pts_off, long long *cnt_off,
                               long long *table_off, long long *total);

/* ---- frames as they arrive: image views in device or host memory ------------------------------------ */
/* A view of one rows x cols image where its producer holds it; nothing is copied to build one.  The packed calls above take one shape only (packed
 * rows, 3-channel colour, uint16 millimetres, a host pointer); a renderer, simulator or decoder on the same GPU, or a torch tensor, delivers RGBA8 /
 * BGRA8 colour, 32FC1 depth in metres, pitched or bottom-up rows, in DEVICE memory.  Formats per image:
 *   depth            TDLO_IMG_U16C1 (millimetres) or TDLO_IMG_F32C1 (metres)
 *   colour           TDLO_IMG_U8C3 or TDLO_IMG_U8C4: the first three bytes of a pixel are the channels, a fourth byte is ignored.  Which channel is which
 *                    stays what tdlo_colour_params.rgb_order says; a view never swaps channels
 *   occluder, mask   TDLO_IMG_U8C1, as in the packed calls
 * The CANONICAL image of a view is the packed, row-major image it stands for: uint16 depth, 3 bytes a pixel of colour, one byte a pixel of occluder or
 * mask.  THE CONTRACT: a view call computes, bit for bit, what the packed call computes from the canonical images (tests/image_view_ref.py is the numpy
 * statement) -- cloud, n, n_raw, node distances, visible sets, the tracker's nodes and sigma2, and the picture tdlo_tracker_render_result draws afterwards.
 * 32FC1 -> millimetres is this library's own rule (the reference reads 16UC1 only, trackdlo_node.cpp:219):
 *   mm = floor(1000 d + 1/2) in exact arithmetic when 0 <= 1000 d + 1/2 < 65536, else 0 (NaN, +-inf, negative values, d >= 65.5355; 0 is the sensor's
 *   "no return", which the path handles already).  It is evaluated as floor((double)d * 1000.0 + 0.5): product and sum are exact in fp64 wherever the
 *   result can depend on them (1000 d >= 0.125; below that the sum stays under 1), so a fused multiply-add cannot change a bit and numpy's
 *   d.astype(float64) * 1000.0 + 0.5 is the same function.  (The float32 form d * 1000.0f + 0.5f is NOT: its result depends on whether the compiler
 *   fuses it.)  k / 1000 rounded to float32 converts back to k for every k in 0 .. 65535: a depth image written in metres reproduces its millimetre image. */
enum { TDLO_IMG_U8C1 = 0, TDLO_IMG_U8C3 = 1, TDLO_IMG_U8C4 = 2, TDLO_IMG_U16C1 = 3, TDLO_IMG_F32C1 = 4 };     /* tdlo_image_view.format */
enum { TDLO_ROLE_DEPTH = 0, TDLO_ROLE_COLOUR = 1, TDLO_ROLE_OCCLUDER = 2, TDLO_ROLE_MASK = 3 };              /* the `role` of tdlo_image_view_check */
typedef struct {
    const void *data;        /* first byte of pixel (0, 0); NULL: this image is absent */
    int format, location;    /* TDLO_IMG_*, TDLO_MEM_AUTO / _HOST / _DEVICE (as tdlo_cloud_view) */
    long long row_stride;    /* BYTES from row r to row r + 1; signed (bottom-up images are images); ROS sensor_msgs/Image.step, cv::Mat::step */
    void *ready_stream;      /* device sources: hipStream_t whose work so far produces the data; NULL = the data is ready */
} tdlo_image_view;
typedef struct { tdlo_image_view depth, colour, occluder, mask; } tdlo_frame_view;
/* Whether (v, rows, cols) describes an image in that role: TDLO_E_INVALID for a null view or null data, an unknown format, location or role, a format
 * the role does not take, data or row_stride that is no multiple of the element size (1, 2 or 4), |row_stride| < cols x bytes per pixel with rows > 1
 * (rows would overlap; with one row any stride is legal), an extent that does not fit 64-bit offsets, rows or cols <= 0, rows x cols > 2^26.  A pitch
 * larger than the row and a negative one are legal.  Needs no context and no GPU; every call below that takes a view runs it first. */
int tdlo_image_view_check(const tdlo_image_view *v, int rows, int cols, int role);
/* The bytes the view addresses, relative to v->data: [*lo_bytes, *hi_bytes) = [min over rows of the row's start, max over rows of the row's start +
 * cols x bytes per pixel).  The library reads no byte outside it, with any load, on host or device (of a pitched image the bytes between the rows lie
 * inside it; they are not read either). */
int tdlo_image_view_extent(const tdlo_image_view *v, int rows, int cols, long long *lo_bytes, long long *hi_bytes);
/* How the import kernel loads a device view, from data, row_stride and cols only: 0 element by element, 1 dword loads, 2 one 8- / 16-byte load per four
 * pixels (csrc/tdlo_image.hip).  Host helper, no device work: exported so that the chooser can be tested on a machine without a GPU. */
int tdlo_image_view_form(const tdlo_image_view *v, int cols);
/* The canonical image of a HOST view, written to canonical_out (rows x cols x {2, 3, 1, 1} bytes by role): what the calls below do with a host view.
 * Host helper, no device work. */
int tdlo_image_view_pack(const tdlo_image_view *v, int rows, int cols, int role, void *canonical_out);
/* tdlo_depth_to_cloud (fv->mask given) or tdlo_colour_depth_to_cloud (fv->colour given; fv->occluder optional; colour_params as there) from views.
 * Both or neither of mask and colour, no depth, a mask together with an occluder, a view that fails tdlo_image_view_check: TDLO_E_INVALID, and nothing
 * of the context -- the slot's cloud, the canonical images -- has been touched.
 *   location  as tdlo_set_cloud_view: TDLO_MEM_AUTO asks the runtime; device memory of another GPU is TDLO_E_INVALID; managed and caller-pinned
 *             memory is host memory.
 *   device sources   ONE kernel launch (k_image_import, csrc/tdlo_image.hip) normalises all of the frame's device images into the context's device
 *             image buffers, where the kernels behind it read them as they do after the copy route; ready_stream: an event recorded on it makes the
 *             context's stream wait for the work that produces the image -- no host wait.
 *   host sources     the host packs and converts the view, row by row, into the context's pinned image buffers (those of tdlo_image_buffers and
 *             tdlo_colour_buffers, whose lifetime rules apply: a view call counts as a call of them), and the call takes their in-place route: one host
 *             pass and no second copy.  (In a frame that mixes host and device images the packed host images are copied to the device buffers.)  A host
 *             view must not lie inside those pinned buffers.
 * The calls are synchronous like the packed ones: the caller's memory is theirs again on return. */
int tdlo_frame_to_cloud_view(tdlo_ctx *ctx, int slot, const tdlo_frame_view *fv, const tdlo_colour_params *colour_params, int rows, int cols,
                             double fx, double fy, double cx, double cy, double leaf_size, double *X_out, int x_capacity, int *n_out, int *n_raw_out);
int tdlo_frame_to_cloud_visibility_view(tdlo_ctx *ctx, int slot, const tdlo_frame_view *fv, const tdlo_colour_params *colour_params, int rows, int cols,
                                        double fx, double fy, double cx, double cy, double leaf_size,
                                        const double *Y, int M, double visibility_threshold, double d_vis, const double *geodesic_coord,
                                        double *node_dist, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                        int *n_out, int *n_raw_out);
/* tdlo_tracker_frame_from_depth (fv->mask given) / tdlo_tracker_frame_from_colour (fv->colour given) from views; a refused frame leaves the tracker's
 * state untouched.  tdlo_tracker_render_result afterwards draws over the canonical colour image of this frame. */
int tdlo_tracker_frame_view(tdlo_tracker *t, const tdlo_frame_view *fv, const tdlo_colour_params *colour_params, int rows, int cols,
                            double fx, double fy, double cx, double cy, double leaf_size, double d_vis,
                            int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                            int *n_out, int *n_raw_out, tdlo_stats *stats);
/* ---- depth aligned to the colour camera, in front of every frame call ----------------------------------- */
/* Every frame call above takes depth and colour (or mask) on ONE pixel grid.  The reference gets that grid from the camera driver: its launch files subscribe
 * to /camera/aligned_depth_to_color/image_raw (launch/trackdlo.launch:6; realsense_node.launch:13 sets align_depth), an image the driver's align filter forms
 * on the CPU.  tdlo_align_depth forms it on the device from the sensor's raw depth stream, so a caller with the two raw streams (or a simulator that renders
 * depth and colour from two cameras) needs no CPU pass over every depth pixel.  The algorithm is the published one of the RealSense SDK's align (depth to
 * another stream); parity against that library is UNPINNED (it is not part of this project's tests), as for OpenCV everywhere else.  THE STATEMENT
 * (tests/align_ref.py is its numpy form, csrc/tdlo_align_lane.h its one text for host and device):
 *   Inputs   a depth image D of rows_d x cols_d (TDLO_IMG_U16C1 millimetres, or TDLO_IMG_F32C1 converted to millimetres by the image views' rule above), the
 *            depth intrinsics (fx_d, fy_d, cx_d, cy_d), the colour camera's size rows_c x cols_c and intrinsics (fx_c, fy_c, cx_c, cy_c), and depth_to_colour:
 *            NULL, or a row-major 3 x 4 matrix T in metres.  No distortion coefficients: both streams are taken as rectified.
 *   Arithmetic   double; every product, quotient and sum is rounded on its own, sums go left to right, NO fused multiply-add anywhere.
 *   Per depth pixel (u, v) with k = D[v, u] != 0:  z = (double)k / 1000.0; for the two corners s = -0.5, +0.5:
 *            x = (((u + s) - cx_d) / fx_d) z, y likewise; q = (x, y, z) if T is NULL, else q_i = ((T_i0 x + T_i1 y) + T_i2 z) + T_i3; the corner is BAD if
 *            q_z <= 0 or any of q is not finite; px = (q_x / q_z) fx_c + cx_c, py likewise; BAD if not |px| < 2^30 or not |py| < 2^30;
 *            X = floor(px + 0.5), Y = floor(py + 0.5) (floor, not the SDK's truncation: the two differ only for -1.5 < px < -0.5, where truncation would let
 *            a footprint reach over the left or top border).  (x0, y0) comes from s = -0.5, (x1, y1) from s = +0.5.  Decisions, IN THIS ORDER:
 *            1 dropped: a corner is bad, or x0 < 0, y0 < 0, x1 >= cols_c, y1 >= rows_c, x1 < x0 or y1 < y0 -- the whole footprint, never clipped;
 *            2 wide:    x1 - x0 + 1 or y1 - y0 + 1 exceeds max_footprint (0 means 16; legal 1 .. 64): a call's time stays bounded;
 *            3 used:    the pixel offers k to every pixel of [y0, y1] x [x0, x1].
 *   Output   A[y, x] = the MINIMUM k offered to the pixel, 0 if none was: a packed rows_c x cols_c uint16 plane.
 *   Counts   counts[4] = {depth pixels with k != 0, used, dropped, wide}.
 * What follows from it: a minimum does not depend on order, so A has one right bit pattern whatever the schedule.  A footprint is about fx_c / fx_d + 1 pixels
 * wide whatever the depth.  Two identical cameras with T = NULL do NOT give D back: the corners land on integers up to rounding, so footprints are 2 - 3
 * pixels wide (580 of the 768 pixels of a random 24 x 32 image differ) -- the algorithm's nature, and the reason the no-FMA rule matters: a corner within one
 * rounding of an integer + 1/2 moves to the next pixel when one multiply-add is fused.  A T that is the identity matrix gives NULL's bits.
 * Out of scope: distortion models, colour aligned to depth.  The form for many cameras in one call -- a rig's K cameras, F frames -- is tdlo_align_depth_batch, below. */
typedef struct {
    int rows_d, cols_d;
    double fx_d, fy_d, cx_d, cy_d;
    int rows_c, cols_c;
    double fx_c, fy_c, cx_c, cy_c;
    const double *depth_to_colour;   /* NULL, or 12 doubles: row-major 3 x 4, metres */
    int max_footprint;               /* 0: 16; else 1 .. 64 */
} tdlo_align_params;
/* TDLO_E_INVALID for null params, sizes that tdlo_image_view_check refuses (rows or cols <= 0, rows x cols > 2^26, of either camera), a focal length that is
 * not finite and positive, a principal point that is not finite, a non-finite matrix entry, max_footprint outside {0, 1 .. 64}.  No context, no GPU. */
int tdlo_align_check(const tdlo_align_params *p);
/* The statement on the host (csrc/tdlo_align_host.cpp, no HIP): depth is a HOST view of rows_d x cols_d (tdlo_image_view_check, role depth); aligned_out
 * takes rows_c x cols_c uint16; counts may be NULL. */
int tdlo_align_depth_host(const tdlo_image_view *depth /* host */, const tdlo_align_params *p, unsigned short *aligned_out, long long counts[4]);
/* The statement on the device: k_align_splat (lane = depth pixel; a returnless 32-bit atomic minimum per offered word of a scratch plane) and k_align_pack
 * (scratch -> uint16, and the scratch armed again), csrc/tdlo_align.hip.  The depth view lies in host or device memory (location and ready_stream as in the
 * view calls above; a host view goes up once, packed); aligned_out: host memory, device memory (2-byte alignment suffices) or NULL; *device_plane
 * (device_plane may be NULL) is the context's aligned plane in device memory, valid until the next align call or a change of size, so that a caller can
 * build a TDLO_MEM_DEVICE depth view on it; counts may be NULL.  One host wait.  TDLO_ALIGN=host, read when the context is made, is the comparator: the plane
 * comes from tdlo_align_depth_host and is uploaded -- the same bits.  tdlo_debug_route_count 59 / 60 count device / host aligns.  A refused call
 * (TDLO_E_INVALID: what tdlo_align_check or tdlo_image_view_check refuse, a pointer on another GPU) has touched nothing. */
int tdlo_align_depth(tdlo_ctx *ctx, const tdlo_image_view *depth, const tdlo_align_params *p, unsigned short *aligned_out,
                     const unsigned short **device_plane, long long counts[4]);
/* tdlo_frame_to_cloud_view / tdlo_tracker_frame_view on two raw streams: fv->depth has the DEPTH camera's size (p->rows_d x p->cols_d); colour, occluder and
 * mask have the colour camera's (p->rows_c x p->cols_c), and the cloud is formed with the colour intrinsics of p.  THE CONTRACT: bit for bit tdlo_align_depth
 * followed by the view call on a TDLO_MEM_DEVICE view of the aligned plane.  The two align launches are enqueued on the context's stream in front of the
 * import: they add NO host wait (TDLO_ALIGN=host adds the host's pass), and counts (may be NULL) come back with the frame's own wait.  A refused call -- bad
 * params, a bad view, a tracker without nodes -- leaves the slot, the tracker, the canonical images and the route counters untouched. */
int tdlo_frame_to_cloud_view_aligning(tdlo_ctx *ctx, int slot, const tdlo_frame_view *fv, const tdlo_align_params *p, const tdlo_colour_params *colour_params,
                                      double leaf_size, double *X_out, int x_capacity, int *n_out, int *n_raw_out, long long counts[4]);
int tdlo_tracker_frame_view_aligning(tdlo_tracker *t, const tdlo_frame_view *fv, const tdlo_align_params *p, const tdlo_colour_params *colour_params,
                                     double leaf_size, double d_vis,
                                     int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                     int *n_out, int *n_raw_out, tdlo_stats *stats, long long counts[4]);
/* ---- raw depth for many cameras in one call: rigs and batches ------------------------------------------------- */
/* Every RGB-D camera has its depth sensor and its colour sensor on different pixel grids, so a rig of K cameras arrives as 2 K raw streams.  tdlo_align_depth
 * serves one camera: K calls are 2 K small launches and K host waits, and each call overwrites the context's one aligned plane.  tdlo_align_depth_batch aligns J
 * JOBS -- a depth view and its params each -- in two launches, the job as the second dimension of the single call's grids (csrc/tdlo_align_batch.hip:
 * k_align_splat_batch, grid (blocks of the job with the most depth pixels, J), and k_align_pack_batch, grid (blocks of the job with the most colour pixels / 4, J);
 * workgroup row j fetches record j of a job table in device memory and runs the single kernels' lanes, csrc/tdlo_align_lane.h unchanged; a workgroup beyond its own
 * job's pixels leaves at once; no grid barrier, no workgroup waits for another), into planes of an ARENA of the context that all stay valid together.
 *   JOBS are independent: each has its own sizes, format (U16 / F32), pitch (positive, negative, padded), location (host / device / auto), ready_stream, transform
 * and max_footprint.  Two jobs may name the same depth view under different params.  A host view goes up once, packed: all host views of a call go into ONE pinned
 * block and ONE copy (a view named by several jobs once).  All device views share one event per distinct ready_stream.
 *   BITS: plane j and counts[4 j .. 4 j + 3] are those of tdlo_align_depth on job j alone, i.e. THE STATEMENT above (tests/align_ref.py: align, counts_of); they
 * depend neither on what else shares the call nor on the order of the jobs.
 *   OUTPUTS: aligned_out: NULL, or J entries, each NULL, host memory or device memory (2-byte alignment suffices) that receives a copy of plane j;
 * device_planes: NULL, or J entries out: plane j in the arena (256-byte aligned, packed rows_c x cols_c uint16); counts: NULL or 4 J; rc_each: NULL or J (a job
 * cannot fail on its own once the call is accepted: zeros).
 *   WAITS: ONE host wait when something must reach the host -- counts non-NULL, or a host aligned_out[j].  Otherwise NO HOST WAIT: the planes are produced on the
 * context's stream (tdlo_stream), and the library guarantees the order by enqueueing on that one stream everything a later call of THIS context does with
 * device_planes[j] -- the rig calls copy a device depth plane on it, the view calls import a TDLO_MEM_DEVICE view on it (ready_stream NULL; a consumer on another
 * stream or context passes ready_stream = tdlo_stream(ctx)), the render batch reads on it.  (A call waits on the host only for the PREVIOUS batch call's uploads to
 * have left the pinned block it is about to rewrite -- long done as a rule; a call that grows the arena drains the stream first.)
 *   LIFETIME: device_planes stay valid, all J together, until the next tdlo_align_depth_batch of the context or one of the aligning rig calls below.  The single
 * call's plane and this arena are independent of each other.
 *   THE ARENA (csrc/tdlo_align_batch_plan.h; tdlo_debug_align_batch_plan): [scratch region | uint16 planes | count words | job table]; scratch planes 16-byte,
 * uint16 planes 256-byte aligned.  Every word of the scratch region is armed (all ones) between calls -- filled when the arena is allocated or the region grows,
 * re-armed by the pack for every plane of the current layout -- so a call whose sizes, order or J differ from the call before needs no fill launch and cannot see
 * a stale word.  J is 1 .. 1024; an arena beyond 1 GiB (kAlignBatchBudget; 64 cameras of 1280 x 720 need about 0.35 GiB) refuses the call.
 *   REFUSED AS A WHOLE with TDLO_E_INVALID before anything is touched, no counter moved: J outside 1 .. 1024; a job that tdlo_align_check or tdlo_image_view_check
 * (role depth, the depth camera's size) refuses; a pointer on another GPU; a device aligned_out[j] or a device view that overlaps the arena; the budget exceeded.
 *   ROUTES (the same bits on each).  kAlignBatchMin (csrc/tdlo_api.cpp) is the smallest J from which a call takes the batch launches; below it the call loops the
 * single launches into the arena's planes -- no host wait either.  NOT MEASURED YET (scripts/gpu_align_batch.py writes profiles/align_batch_ab.txt; the rule, set
 * beforehand: the smallest J from which every batch value lies below every looped value on all four lines -- 640 x 480 -> 640 x 480 and 848 x 480 -> 1280 x 720,
 * device and pageable host depth --, 1025 if no J up to 32 qualifies): until it is, kAlignBatchMin is 1025 and BY DEFAULT THE CALL LOOPS THE SINGLE LAUNCHES.
 * TDLO_ALIGN_BATCH_MIN=n, read when the context is made, overrides it.  TDLO_ALIGN=host forms every plane with tdlo_align_depth_host and uploads it.
 * tdlo_debug_route_count 61 counts the jobs the batch launches served, 62 the jobs the looped single launches served; 59 / 60 keep counting what the single
 * launches / the host statement did (a looped job moves 59 and 62); 63 counts the DISTINCT jobs formed inside the aligning rig calls below.
 * Out of scope: an aligning form of tdlo_tracker_frame_views_batch -- the no-wait call and TDLO_MEM_DEVICE views of device_planes compose it by hand --, the pack
 * writing straight into the rig arena. */
typedef struct { tdlo_image_view depth; tdlo_align_params p; } tdlo_align_job;
int tdlo_align_depth_batch(tdlo_ctx *ctx, const tdlo_align_job *jobs, int J,
                           unsigned short *const *aligned_out   /* NULL, or J entries: NULL / host / device memory */,
                           const unsigned short **device_planes /* NULL, or J entries out: the arena's planes */,
                           long long *counts /* NULL or 4 J */, int *rc_each /* NULL or J */);
/* The rig calls from raw streams.  cams[k].depth must be NULL; raw[k] is camera k's raw depth view and its align params, whose colour size is the rig's
 * rows x cols.  THE CONTRACT: bit for bit the composition by hand -- tdlo_align_depth per camera, each plane kept, then the existing rig call (tdlo_rig_to_cloud,
 * tdlo_tracker_frame_from_rig, tdlo_tracker_frames_from_rig_batch) with those planes as device depth planes: the cloud, n, n_raw, the visible sets, the nodes and
 * sigma2, under the existing calls' own conditions.  These entrances CALL the existing calls, so the routes and the rig self-occlusion switch behave as there.
 *   DISTINCT JOBS: two (camera, frame) entries with equal view fields (data, format, row_stride, location, ready_stream) and bytewise-equal params (the matrix
 * compared by value) are ONE job: F ropes under one rig align K planes, not F K (tdlo_debug_route_count 63 counts them; at most 1024 a call).  counts (NULL, or
 * four per (frame, camera) entry, frame after frame) still has one row per entry.
 *   WAITS: the align launches go in front of the rig call's copies on the context's stream and add no host wait; counts come back with the rig call's own wait.
 *   A REFUSED call leaves slots, trackers, the arena's planes and all counters untouched: a camera with depth non-NULL, a raw[k].p whose colour size is not
 * rows x cols, and everything tdlo_align_depth_batch and the existing rig call refuse. */
int tdlo_rig_to_cloud_aligning(tdlo_ctx *ctx, int slot, const tdlo_rig_camera *cams, const tdlo_align_job *raw, int K, int rows, int cols,
                               double leaf_size, double *X_out, int x_capacity, int *n_out, int *n_raw_out, long long *counts /* NULL or 4 K */);
int tdlo_tracker_frame_from_rig_aligning(tdlo_tracker *t, const tdlo_rig_camera *cams, const tdlo_align_job *raw, int K, int rows, int cols,
                                         double leaf_size, double d_vis,
                                         int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                         int *n_out, int *n_raw_out, tdlo_stats *stats, long long *counts /* NULL or 4 K */);
typedef struct { int slot; const tdlo_rig_camera *cams; const tdlo_align_job *raw; int K; } tdlo_rig_raw_frame;
int tdlo_tracker_frames_from_rig_aligning_batch(tdlo_tracker *const *trackers, int F, const tdlo_rig_raw_frame *frames /* .slot not read */,
                                                int rows, int cols, double leaf_size, double d_vis,
                                                int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                                int *n_out, int *n_raw_out, tdlo_stats *stats /* 2 F */, int *rc_each, long long *counts /* NULL or 4 sum K_f */);
/* The arena layout of csrc/tdlo_align_batch_plan.h (no context, no GPU), shaped like tdlo_debug_rig_batch_plan: J jobs of rows_c[j] x cols_c[j] colour pixels;
 * budget: the bytes the arena may take (<= 0: the library's 1 GiB).  Outputs in bytes from the arena's start, any may be NULL: scratch_off / plane_off / counts_off:
 * J entries (job j's scratch plane, uint16 plane, four count words); *table_off; *scratch_bytes: the scratch region is [0, scratch_bytes); *total.
 * TDLO_E_INVALID: J outside 1 .. 1024, a size below 1 or beyond 2^26 pixels, a total beyond the budget.  tdlo_debug_align_batch_arena: where the context's
 * align-batch arena lies at present (a test aid for the overlap refusal; NULL / 0 before the first batch).  tdlo_debug_align_distinct_jobs: the distinct-job rule
 * on n (view, params) entries -- job_of[e] is the index of entry e's job in order of first appearance; returns the number of distinct jobs, or a negative code. */
int tdlo_debug_align_batch_plan(const int *rows_c, const int *cols_c, int J, long long budget, long long *scratch_off, long long *plane_off,
                                long long *counts_off, long long *table_off, long long *scratch_bytes, long long *total);
int tdlo_debug_align_batch_arena(tdlo_ctx *ctx, const void **base, long long *bytes);
int tdlo_debug_align_distinct_jobs(const tdlo_align_job *entries, int n, int *job_of);
/* ---- image views for many slots in one call ----------------------------------------------------------- */
/* tdlo_depth_to_cloud_batch for callers who come with image VIEWS: a simulator, renderer or decoder on the same GPU that makes K camera images as one device
 * tensor ([K, H, W, 4] uint8 and [K, H, W] float32) and steps as many trackers.  An IMAGE is a tdlo_frame_view -- depth, and a mask, or a colour view (with
 * an optional occluder), or both -- and its intrinsics; FRAMES and their sharing are those of the packed batch: colour_params == NULL takes the image's mask,
 * otherwise the segmentation is formed from its colour view under these ranges; any number of frames may name one image, each with its own ranges.
 *   BITS: every slot's cloud, n_out[f] and n_raw_out[f] are those of tdlo_frame_to_cloud_view on that frame alone (i.e. what the packed call computes from
 * the canonical images of tests/image_view_ref.py), the sign of a zero included, whatever else shares the call and in whatever order.
 *   PLANES: only views a frame reads are imported, every distinct (data, format, row_stride, role) once, into the arena of the packed batch.  Device views
 * are written there by ONE launch of k_image_import_batch (csrc/tdlo_image.hip: grid (blocks of an image's lanes, images); a job of its table is one image,
 * the load form per view as tdlo_image_view_form gives it; no load touches a byte outside a view's extent; no workgroup waits for another), behind one event
 * per distinct ready_stream.  Host views are packed by the host into one pinned block laid out as their arena region and go up, together with the two tables,
 * in ONE copy.  Per call, then: at most one copy, one import launch, at most two k_cloud_fused_batch launches and one host wait.
 *   ROUTES: below the crossover (next paragraph), with TDLO_CLOUD_FUSED off or for an image size the one-launch cloud kernel does not take, the call loops
 * over tdlo_frame_to_cloud_view.  A frame the cloud kernel passes on (more than 32 704 masked pixels, word-layout limits, pass-through) goes through the
 * single view call for its slot alone; its code goes to rc_each, and the call returns the first non-zero code.  tdlo_debug_route_count 42 counts the frames
 * the batch launches served, 43 the frames passed on or looped, 44 the planes k_image_import_batch wrote; 6 / 7 / 15 .. 18 keep counting what the single
 * route does, and 32 / 33 (the packed batch's) do not move.
 *   CROSSOVER: kFrameViewBatchMin for this call, kFrameViewBatchTrackerMin for the tracker call (csrc/tdlo_api.cpp), by the rule set beforehand -- the
 * smallest F from which every batch value lies below every single-calls value on the lines a call stands for, at 640 x 480 and 1280 x 720
 * (scripts/gpu_frame_view_batch.py -> profiles/frame_view_batch_ab.txt).  MEASURED against F single view calls through the parent commit's library (rope
 * frames, F = 1 .. 32, five alternating rounds of 20 calls): one frame costs more as a batch (0.075 against 0.044 ms at 640 x 480, 0.142 against 0.057 ms at
 * 1280 x 720); DEVICE views win on every value from 2 frames at 640 x 480 and from 4 at 1280 x 720 -- 32 RGBA8 + 32FC1 images 0.20 against 1.42 ms and 0.58
 * against 1.84 ms, bgr8 + 16UC1 the same -- but HOST views, packed and copied up, stay behind single calls that read the context's pinned buffers in place at
 * every F at 1280 x 720 (32 images 9.6 against 7.3 ms; at 640 x 480 they win at some F and lose at others).  So the rule gives kFrameViewBatchMin = 33:
 * BY DEFAULT tdlo_frame_views_to_cloud_batch LOOPS OVER THE SINGLE VIEW CALLS, and TDLO_FRAME_VIEW_BATCH_MIN=n (read when the context is made) turns the batch
 * launches on from n frames -- worth it for callers whose views lie in device memory.  The tracker call (measured on device views) wins on every value from 4
 * trackers on at both sizes -- 32 trackers 2.13 against 5.69 ms at 640 x 480, 2.29 against 5.74 ms at 1280 x 720 -- so kFrameViewBatchTrackerMin = 4.
 *   Refused as a whole with TDLO_E_INVALID before anything is touched (resident clouds intact, no counter moved): what tdlo_depth_to_cloud_batch refuses;
 * per view what tdlo_image_view_check refuses; an occluder without a colour view; a pointer on another GPU; a host view inside the context's pinned image
 * buffers; a device view that overlaps the batch arena or the resident cloud of any slot the call names.
 *   NOT DONE HERE (follow-ups): k_cloud_fused_batch reading the views in place, which would save the import's round trip through the arena (the bytes per
 * call in the profile file are what that decision rests on); the packed batch's device planes through k_image_import_batch; any change to kCloudBatchMin. */
typedef struct { tdlo_frame_view fv; double fx, fy, cx, cy; } tdlo_view_image;
int tdlo_frame_views_to_cloud_batch(tdlo_ctx *ctx, const tdlo_view_image *images, int K, int rows, int cols,
                                    const tdlo_batch_frame *frames, int F, double leaf_size,
                                    int *n_out /* F */, int *n_raw_out /* F */, int *rc_each /* F or NULL */);
/* The call above into the trackers' slots (under kFrameViewBatchTrackerMin), then tdlo_tracker_frame_batch on the trackers whose cloud is not empty: the
 * bits of the two, under tdlo_tracker_frame_batch's stated conditions.  Arguments, outputs, TDLO_E_EMPTY and refusals as for tdlo_tracker_frames_batch. */
int tdlo_tracker_frame_views_batch(tdlo_tracker *const *trackers, int F, const tdlo_view_image *images, int K, int rows, int cols,
                                   const int *image_of /* F */, const tdlo_colour_params *const *colour_params /* NULL or F entries, each NULL = mask */,
                                   double leaf_size, double d_vis,
                                   int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                   int *n_out, int *n_raw_out, tdlo_stats *stats, int *rc_each);
/* The device addresses of image k's canonical planes (tightly packed rows x cols x {2, 3, 1, 1} bytes, 256-byte aligned) in the arena, as the most recent
 * view batch on the context left them; a plane that call did not import -- no frame read it, or the call looped over the single calls -- is NULL.  Any output
 * may be NULL.  The pointers are valid until the next batch call (packed or views) on the context.  The colour plane is what a caller who came with RGBA views
 * hands to tdlo_tracker_render_result_batch, which reads 4-byte aligned device memory in place.  TDLO_E_INVALID: no such call yet, or k out of range. */
int tdlo_view_batch_images(tdlo_ctx *ctx, int k, const unsigned short **depth, const unsigned char **colour,
                           const unsigned char **occluder, const unsigned char **mask);
/* Test aid: where the slot's resident cloud lies in device memory (NULL: none yet) and how many points the block holds (3 x capacity doubles) -- the memory
 * a device view must not overlap.  Either output may be NULL. */
int tdlo_debug_slot_cloud(tdlo_ctx *ctx, int slot, const double **X, int *capacity);

/* Test aid: copies out the canonical images the context's last view call left (device buffers or the pinned ones), each to a host buffer that may be
 * NULL.  TDLO_E_INVALID when there was no such call, its shape differs, or an image is asked for that the frame did not have. */
int tdlo_debug_read_images(tdlo_ctx *ctx, int rows, int cols, unsigned short *depth_out, unsigned char *colour_out, unsigned char *occluder_out,
                           unsigned char *mask_out);

/* ---- the tracking-result image on the device: blend, edges and nodes in one kernel ----------------- */
/* The picture the node publishes every frame (trackdlo/src/trackdlo_node.cpp:377-452), so that a caller of tdlo_tracker_frame_from_colour needs no OpenCV
 * pass on the host for it either (a full-image cv::addWeighted, M - 1 cv::line and 2 (M - 1) cv::circle calls).  Stated exactly:
 *   blend   per byte, a = the colour byte, b = a & o (o: the pixel's occluder byte, 255 without an occluder -- the reference ANDs with a BGR occlusion
 *           image, this library's occluder is one byte per pixel): s = a + b, out = (s >> 1) + ((s & 1) & ((s >> 1) & 1)), i.e. 0.5 a + 0.5 b rounded half
 *           to even, what cv::addWeighted does for 8-bit images (cvRound);
 *   pixels  node m -> u = ((p0 x + p1 y) + p2 z) + p3, v, w likewise (fp64), col = (int)(u / w), row = (int)(v / w).  w <= 0, a non-finite quotient or a
 *           pixel coordinate outside [-8192, 8191]: TDLO_E_INVALID, nothing is drawn, the output is untouched; so are images beyond 8192 rows or columns;
 *   order   edge i joins nodes i and i + 1; key sqrt(mx^2 + my^2 + mz^2) of its mid-point m = (Y_i + Y_i+1) / 2; ascending by (key, i), then REVERSED:
 *           the farthest edge first (:378-390);
 *   per edge, in that order: a line from pixel i to pixel i + 1 of line_width (every pixel within line_width / 2 of the segment between the end pixels,
 *           in exact integers: the rule of the self-occlusion test below), the disc of node i, the disc of node i + 1 (dx^2 + dy^2 <= node_radius^2);
 *   colours node k: node_visible when k is in vis, else node_hidden; edge i: edge_hidden only when neither i nor i + 1 is in vis, else edge_visible
 *           (:409-424).  A later primitive overwrites an earlier one; primitives are clipped to the image; one node draws nothing (the blend alone).
 * PARITY UNPINNED against OpenCV: line and disc are their geometric content, not OpenCV's own fixed-point rasterisers (OpenCV is not part of the build
 * image; boundary pixels may differ), like the painter test and the colour routine; tests/render_ref.py is the numpy statement the kernel is held to byte
 * for byte.  NOT drawn: the text label cv::putText(... "occlusion" ...) of :446-449 -- its Hershey font is OpenCV's data.  The occlusion corners it is
 * placed by (:198-208) are returned instead, so that the caller can place the label: corners = {row, col of the first pixel in row-major order whose
 * occluder byte is 0, row, col of the last one}, all -1 when there is none or no occluder. */
typedef struct {
    int line_width, node_radius;              /* 1 .. 255 each; the reference: 5 and 7 */
    unsigned char node_visible[3], node_hidden[3], edge_visible[3], edge_hidden[3];      /* in the image's byte order; the reference (bgr8):
                                                                                           * {0,150,255}, {0,0,255}, {0,255,0}, {0,0,255} */
} tdlo_render_params;
void tdlo_default_render_params(tdlo_render_params *p);
/* The host half, no device work (exported like the other host helpers so that a test can address it on a machine without a GPU).  prims: room for
 * 3 (M - 1) records of 8 ints {kind 0 line / 1 disc, c0, r0, c1, r1 (a disc: its centre twice), size (width / radius), colour b | g << 8 | r << 16, 0} in
 * drawing order; *n_prims = 3 (M - 1).  p == NULL: the defaults.  vis entries outside 0 .. M - 1, a size outside 1 .. 255, a node that cannot be drawn:
 * TDLO_E_INVALID, prims untouched. */
int tdlo_render_primitives(const double *Y, int M, const double proj[12], const int *vis, int n_vis, const tdlo_render_params *p, int *prims, int *n_prims);
/* A pinned host buffer of the context for a rows x cols x 3 result image, with the lifetime rules of tdlo_colour_buffers.  Passed as image_out, it is
 * written by the kernel itself, over PCIe -- no device-to-host copy behind the kernel. */
int tdlo_result_image_buffer(tdlo_ctx *ctx, int rows, int cols, unsigned char **image);
/* One launch (k_render, csrc/tdlo_render.hip) and the call returns when the image is complete.
 *   colour     rows x cols x 3 uint8, staged exactly as the colour calls stage it (tdlo_colour_buffers' pointers are read in place), occluder rows x cols or
 *              NULL.  colour == NULL: the colour and occluder images of the context's most recent colour call (tdlo_colour_mask, tdlo_colour_depth_to_cloud*,
 *              tdlo_tracker_frame_from_colour, or an earlier tdlo_render_result that was given a colour image: it stages one like the others), read
 *              where that call left them -- its device copy, or the pinned buffers as they are NOW -- with no second upload; the occluder argument is
 *              ignored.  TDLO_E_INVALID when there was no such call or its shape differs (tdlo_last_colour_shape tells the shape).
 *   Y, M       1 .. 1024 nodes, column-major; proj 3 x 4 row-major; vis, n_vis: the index set behind the colours.
 *   image_out  rows x cols x 3: pageable host memory, tdlo_result_image_buffer's pointer, or device memory of the context's GPU (asked of the runtime
 *              as tdlo_set_cloud_view asks).  The kernel writes the latter two itself; a device pointer that is not 4-byte aligned receives a copy.
 *              TDLO_RENDER_INPLACE=0, read when the context is made: the kernel always writes a device image of the context that is then copied out
 *              -- the comparator, the same bytes (tdlo_debug_route_count 19 / 20).
 *   corners    may be NULL.
 * Every refusal leaves image_out untouched. */
int tdlo_render_result(tdlo_ctx *ctx, const unsigned char *colour, const unsigned char *occluder, int rows, int cols,
                       const double *Y, int M, const double proj[12], const int *vis, int n_vis,
                       const tdlo_render_params *p /* NULL: defaults */, unsigned char *image_out, int corners[4] /* may be NULL */);
/* The shape of the context's most recent colour call, i.e. what tdlo_render_result with colour == NULL and tdlo_tracker_render_result draw over and the
 * shape their image_out has.  TDLO_E_INVALID (rows and cols untouched) when there was none.  No device work. */
int tdlo_last_colour_shape(tdlo_ctx *ctx, int *rows, int *cols);
/* The tracker's current nodes (the result of its last step) over the last colour frame of its context (colour == NULL above).  vis is the reference's
 * not_self_occluded_nodes (:401): with tdlo_tracker_set_self_occlusion on, the nodes that test leaves with an infinite distance threshold, formed from the
 * nodes the last tdlo_tracker_frame_from_* call STARTED from, as the callback does at :279-343; off: every node.  proj == NULL: the matrix given to
 * tdlo_tracker_set_self_occlusion, else {fx, 0, cx, 0,  0, fy, cy, 0,  0, 0, 1, 0} from the last frame call's intrinsics.  The tracker's state is not
 * touched: a tracker that renders and one that does not give the same nodes, bit for bit. */
int tdlo_tracker_render_result(tdlo_tracker *t, const double proj[12], const tdlo_render_params *p, unsigned char *image_out, int corners[4]);

/* Result images for many ropes: any number of ropes over each image, K images of one size in ONE launch (k_render_batch, csrc/tdlo_render_batch.hip).
 * tdlo_render_result blends the whole image and paints its one rope, so a picture of several ropes over one camera image cannot be made from single calls
 * (a second call over the first one's output blends twice, over the original it loses the first rope).  Per image k, in terms of the single call:
 *     img = blend(colour_k, occluder_k)
 *     for every rope whose .image == k, in the order of the caller's rope list: if rope.M > 1, paint its primitives (tdlo_render_primitives) over img
 *     corners_k = the occlusion corners of occluder_k
 * i.e. the blend ONCE, then each rope exactly as tdlo_render_result draws its one rope (edges farthest first: line, disc, disc; the same pixel rule, the
 * same guards); ropes in list order, so a later rope paints over an earlier one -- what R successive drawing passes over one blended image give, and
 * the caller controls it.  An image without a rope is the blend alone; an image with exactly one rope is byte for byte tdlo_render_result's.
 * PARITY UNPINNED against OpenCV's own rasterisers, exactly as for the single call; tests/render_batch_ref.py is the numpy statement.
 *   limits     1 .. 256 images of 1 .. 8192 rows and columns, 0 .. 1024 ropes of 1 .. 1024 nodes; the device and pinned tables grow on demand.
 *   sources    as the single call's: the context's pinned colour buffers (tdlo_colour_buffers) and 4-byte aligned device memory of the context's GPU are read
 *              in place; pageable host memory and unaligned device memory are staged into a device arena of the context.  colour == NULL: the images of
 *              the context's most recent colour call, as tdlo_render_result (occluder is ignored then).
 *   image_out  per image: 4-byte aligned device memory of the context's GPU and tdlo_result_image_buffer's pointer are written by the kernel; anything else
 *              is written into the arena and copied out behind the launch.  With 3 rows cols not a multiple of 4, consecutive images of one device tensor
 *              alternate between the two routes.  TDLO_RENDER_INPLACE=0: the arena and a copy for every image.  tdlo_debug_route_count 34 counts the images
 *              the kernel wrote in place, 35 the images copied out of the arena (19 / 20 stay the single call's).
 *   corners    4 K ints (image k: corners[4 k ..]) or NULL.
 * All or nothing: TDLO_E_INVALID, tdlo_last_error names the rope or image, and NO byte of any image_out and no entry of corners is written -- a rope
 * whose image is outside 0 .. K - 1, a rope tdlo_render_primitives refuses, a NULL image_out, two images with the same image_out, colour == NULL without
 * a colour call of the same shape before it, device memory of another GPU.
 * One launch per call, plus the table upload, the corner words' memset, the copies of staged sources and arena images, one read-back of the corner words
 * and one stream wait.  Cost (profiles/render_batch_ab.txt, measured against K x tdlo_render_result, medians): one image costs what the single call
 * costs (640 x 480: 0.068 against 0.068 ms device-resident, 0.201 against 0.199 pageable both ways); from K = 2 on the batch is cheaper on every line
 * (K = 32: 0.53 against 2.01 ms and 3.87 against 7.00 ms; 1280 x 720: 0.70 against 1.89 and 4.54 against 7.54 ms).  There is no routing threshold: the calls
 * always take k_render_batch. */
typedef struct { const unsigned char *colour;    /* rows x cols x 3, or NULL: the context's most recent colour frame (as tdlo_render_result) */
                 const unsigned char *occluder;  /* rows x cols or NULL; ignored when colour == NULL */
                 unsigned char *image_out;       /* rows x cols x 3 */ } tdlo_render_image;
typedef struct { int image, M; const double *Y /* column-major, 3 M */; const double *proj /* 12 */;
                 const int *vis; int n_vis; const tdlo_render_params *params /* NULL: defaults */; } tdlo_render_rope;
/* The host half, no device work: the table the kernel reads.  Ropes are ordered stably by image: positions rope_first[k] .. rope_first[k + 1] - 1 are image
 * k's ropes in list order (rope_first: K + 1 ints).  heads: eight ints per rope, in that order: {c_lo, r_lo, c_hi, r_hi, first primitive, number of
 * primitives, 0, 0} -- the union of its primitives' bounding boxes, a disc inflated by its radius, a line by (width + 1) >> 1; a one-node rope has no
 * primitive and the empty box {0, 0, -1, -1}.  prims: tdlo_render_primitives' records, rope after rope in the same order; *n_prims their number.
 * TDLO_E_INVALID (every output untouched): R outside 0 .. 1024, K outside 1 .. 256, a rope's image outside 0 .. K - 1, a rope of fewer than 1 or more
 * than 1024 nodes or one that tdlo_render_primitives refuses, more than prims_cap records. */
int tdlo_render_batch_table(const tdlo_render_rope *ropes, int R, int K,
                            int *heads /* 8 R ints */, int *prims /* 8 ints per primitive */, int prims_cap, int *n_prims, int *rope_first /* K + 1 */);
int tdlo_render_result_batch(tdlo_ctx *ctx, const tdlo_render_image *images, int K, int rows, int cols,
                             const tdlo_render_rope *ropes, int R, int *corners /* 4 K or NULL */);
/* Rope i: tracker i's current nodes over image image_of[i], vis formed exactly as tdlo_tracker_render_result forms it; proj_each / params_each: NULL, or F
 * entries of which any may be NULL (the tracker's matrix as tdlo_tracker_render_result chooses it / the default parameters).  The images are passed
 * explicitly, as tdlo_tracker_frames_batch takes them: a batch of cloud calls leaves no per-image colour residency to lean on.  Refused as above, and for
 * trackers of different contexts or a tracker without nodes.  No tracker's state is touched. */
int tdlo_tracker_render_result_batch(tdlo_tracker *const *trackers, int F, const tdlo_render_image *images, int K, int rows, int cols,
                                     const int *image_of /* F */, const double *const *proj_each /* F entries or NULL; an entry may be NULL */,
                                     const tdlo_render_params *const *params_each /* likewise */, int *corners /* 4 K or NULL */);

/* The callback's self-occlusion ("painter") test, trackdlo/src/trackdlo_node.cpp:279-343: the edges between consecutive nodes are taken nearest the camera
 * first (:279-290, by the camera distance of their mid-points) and each is drawn as a line of dlo_pixel_width pixels (:337-341) after its two end nodes
 * were looked up in what had been drawn before (:304-334): a node whose projected pixel (proj: 3 x 4 row-major, the reference's proj_matrix; pixel
 * coordinates truncated as by static_cast<int>) lies under an edge nearer than its own is left out; the others are visible when they are within
 * visibility_threshold of the cloud (node_dist[M]: what tdlo_visibility_prepass / tdlo_depth_to_cloud_visibility return, :257-277).  visible_nodes
 * receives the ascending indices (room for M ints), *n_vis their number.  Host code, O(M^2) integer tests, no device work.
 * PARITY UNPINNED against OpenCV: "under an edge" is the geometric content of cv::line with a thickness -- within dlo_pixel_width / 2 of the segment
 * between the end pixels --, not OpenCV's own fixed-point rasteriser (absent from the build image); boundary pixels may differ.  tests: the oracle's
 * literal restatement of the callback's loop (oracle/ref_cpu.c, ref_self_occlusion) gives the same index sets on random self-crossing ropes. */
int tdlo_self_occlusion_visible(const double *Y, int M, const double proj[12], int dlo_pixel_width, const double *node_dist, double visibility_threshold,
                                int *visible_nodes, int *n_vis);
/* trackdlo_node.cpp:345-360: visible_nodes sorted, occluded runs shorter than d_vis (in geodesic_coord) filled in.  Room for the chain's node count. */
int tdlo_extend_visible_nodes(const int *visible_nodes, int n_vis, const double *geodesic_coord, double d_vis, int *visible_nodes_extended, int *n_vis_ext);
/* tdlo_tracker_frame_from_depth applies the self-occlusion test above between its distance pre-pass and the gap fill (the reference callback's order)
 * once the tracker has been given the projection matrix and the rope's width in pixels; proj == NULL switches it off again.  OFF by default (see the
 * parity note above). */
int tdlo_tracker_set_self_occlusion(tdlo_tracker *t, const double *proj, int dlo_pixel_width);

/* ---- host helpers on the path (exported so the parity tests can address them directly) -------- */
/* trackdlo::calc_LLE_weights (trackdlo.cpp:119-159), k as passed at :236 (6). L: M x M col-major out. */
int tdlo_calc_lle_weights(int k, const double *Y, int M, double *L);
/* H = (I - L)^T (I - L) of trackdlo.cpp:236-237 (L = calc_LLE_weights with k = 6) as the registrations form it: H (M x M col-major, optional) by
 * the dense route that the dense LLE M-steps use, Hb (13 M, optional; Hb[13 i + u] = H(i, i - 6 + u)) by the O(M) route of the banded LLE
 * M-step -- the same values bit for bit (tests/test_abi.py). */
int tdlo_calc_lle_regulariser(const double *Y, int M, double *H, double *Hb);
/* line_sphere_intersection (trackdlo/src/utils.cpp:185-241): returns number of points (0..2) */
int tdlo_line_sphere_intersection(const double A[3], const double B[3], const double C[3],
                                  double radius, double out[6]);
/* trackdlo::traverse_euclidean (trackdlo.cpp:584-898): returns number of pairs or TDLO_E_TRAVERSE */
int tdlo_traverse_euclidean(const double *geodesic_coord, int n_coord, const double *guide_nodes, int Mg,
                            const int *visible_nodes, int n_vis, int alignment, int alignment_node_idx,
                            double *out /* (n_coord + 2) x 4 row-major */);

/* ---- frame-level accuracy metric ------------------------------------------ */
/* evaluator::get_piecewise_error (trackdlo/src/evaluator.cpp:258-283, with calc_min_distance :233-256): mean over the
 * nodes of Y_track of the distance to the polyline through Y_true.  Chains are n x 3 column-major.  < 0 on bad input. */
double tdlo_piecewise_error(const double *Y_track, int n_track, const double *Y_true, int n_true);
/* evaluator::compute_error (evaluator.cpp:333-341): the symmetrised mean (E(track,true) + E(true,track)) / 2. */
double tdlo_compute_error(const double *Y_track, int n_track, const double *Y_true, int n_true);

/* ---- measurement ------------------------------------------------------------------------------ */
/* Launches the E-step kernel `reps` times back to back on the context's stream for the state left
 * by the last cpd_lle call on `slot` and returns the HIP-event average per launch (microseconds).
 * kind: 0 = membership/E-step kernel, 1 = per-node min-distance kernel, 2 = M-step kernel;
 * kind 10 = the E-step IN SITU: `reps` (<= 256) real iterations (E-step and M-step alternating as in the loop), each
 * E-step dispatch carrying its own start/stop events (hipExtLaunchKernelGGL) -- the per-dispatch duration a kernel
 * trace reports, measured live on the context's stream. */
int tdlo_profile_kernel(tdlo_ctx *ctx, int slot, int kind, int reps, float *avg_us);
/* One EM iteration IN SITU on the state left by the last cpd_lle call (all frames of the last call): `reps` (<= 256) real
 * iterations on the context's stream; the E-step dispatch and the M-step dispatch of every iteration carry their own HIP
 * start/stop events (hipExtLaunchKernelGGL) -- the per-dispatch durations a kernel trace reports.  *iter_us = stream time
 * per whole iteration (dispatch gaps and the small kernels of the visibility / large-cloud paths included).
 * mstep_kernel receives the name of the M-step kernel these frames dispatch; *mstep_us = -1 when that kernel's dispatch
 * carries no events (the pivoted paths). */
int tdlo_profile_iteration(tdlo_ctx *ctx, int reps, float *estep_us, float *mstep_us, float *iter_us, char *mstep_kernel, int name_cap);
/* Development aid: copies the first n (<= 64) shader-clock stamps that the M-step kernel of the last
 * launch wrote at its phase boundaries (reduce / assemble / eliminate / update / publish). */
int tdlo_debug_stamps(tdlo_ctx *ctx, int slot, unsigned long long *out, int n);
/* Test aid: y[i] = 2^x[i] as the fp64 E-step computes it (its own 17-instruction form, csrc/tdlo_devcommon.h: Num<double>::exp2, not the
 * library's); host arrays of n doubles. */
int tdlo_debug_exp2(tdlo_ctx *ctx, const double *x, double *y, int n);
/* Test aid: which M-step serves registrations WITHOUT the LLE term from now on, process-wide.  0 (default): the chain smoother
 * (csrc/tdlo_mstep_chain.hip: the system of trackdlo.cpp:405-413 solved in O(M) through the state-space form of the kernel G);
 * 1: the dense eliminations of the same system (k_mstep_fast / k_mstep_mcu), kept as comparators.  Returns the previous
 * setting.  The initial setting is 1 when the environment holds TDLO_MSTEP=dense. */
int tdlo_debug_mstep_dense(int on);
/* Test aid: which M-step serves registrations WITH the LLE term (include_lle: the pre-processing registration of tracking_step,
 * trackdlo.cpp:925-927) from now on, process-wide.  0 (default): the banded L D L^T of the system of :396-415 in the state (f, f') of
 * the chain (csrc/tdlo_mstep_band.hip, O(M)), wherever the chain and H allow it -- no two consecutive nodes closer than about a
 * millimetre, H banded like the reference's own (I - L)^T (I - L); 1: always the dense pivoted eliminations (k_mstep_fast<pivoted> /
 * k_mstep / k_mstep_pivot_mcu), kept as comparators and for everything the banded form does not take.  Returns the previous setting.
 * The initial setting is 1 when the environment holds TDLO_MSTEP_LLE=dense. */
int tdlo_debug_mstep_lle_dense(int on);
/* How many calls of this context were repeated on the dense pivoted kernels because the banded L D L^T (which takes no pivots) met a
 * non-positive pivot or produced a non-finite sigma2: an indefinite H_override, or a chain at the edge of the gap test.  The reference's
 * solver is a general one (trackdlo.cpp:415); the caller sees the dense kernels' result, and tdlo_stats.band_retry = 1 on that call
 * (tdlo_cpd_lle*, tdlo_split_run in both forms: the ranks solve the same system and repeat together).  fp64 mode adds one more reason: a
 * sigma2 above 6.25e7 h^3 / beta^4 m2 (h = the chain's mean link length; 0.8 m2 at beta = 5 and 2 cm links, 6e4 m2 at the reference's
 * beta = 0.35) -- met only when a registration starts from sigma2 = 0 on a chain many metres long -- where the state precision's entries,
 * rounded to fp64, leave the banded result a few 1e-9 m from the dense system's; a sigma2 GIVEN above the bound takes the dense kernels
 * without a first attempt (no retry counted).  -1 for a null context. */
long long tdlo_debug_band_retries(tdlo_ctx *ctx);
/* Test aid: the 13 diagonals of H = (I - L)^T (I - L) (see tdlo_calc_lle_regulariser) formed by the DEVICE routine that tdlo_tracker_tracking_step's
 * main registration ends with (csrc/tdlo_lle_dev.h; 1 .. 256 nodes): Hb[13 i + u] = H(i, i - 6 + u), the host routine's values bit for bit. */
int tdlo_debug_lle_band_device(tdlo_ctx *ctx, const double *Y, int M, double *Hb);
/* Test aid: how often tdlo_tracker_tracking_step took its short cuts on this context (none changes a bit of any result; each has an environment
 * switch that turns it off, read when the context is made).  which = 0: main registrations whose node-side set-up had ridden in the
 * pre-processing registration's prologue (every node visible; TDLO_PAIR_SETUP=0); 1: ... that started from the first E-step's sums handed over
 * by the pre-processing registration instead of repeating that E-step (TDLO_PAIR_SUMS=0); 2: ... whose first M-step had been launched ahead of
 * its priors and was released when they were staged (TDLO_SPEC_MSTEP=0); 3: pre-processing registrations whose LLE regulariser had been formed
 * on the device by the M-step that finished the previous frame (TDLO_LLE_NEXT=0); 4: main registrations of frames with hidden nodes whose first
 * iteration had run on the second stream beside the pre-processing registration (TDLO_AHEAD=0); 5: calls repeated on the three-kernel route because
 * the fused prologue's grid barrier was abandoned; 6 / 7: tdlo_depth_to_cloud calls served by the one-launch kernel / passed on by it to the
 * multi-launch form; 8: frames whose visibility pre-pass rode in the depth -> cloud launch (tdlo_depth_to_cloud_visibility); 9: registrations whose
 * E-step was k_estep2 -- two points per lane, csrc/tdlo_estep2.hip: fp32 mode, chains of 8 .. 64 nodes, a cloud or a batch of at least 2048 x 64
 * points, i.e. one that fills the GPU (TDLO_ESTEP2=0: k_estep everywhere, the comparator; =1: wherever eligible, whatever the size).  The two
 * E-step kernels differ in the grain of their fp32 tile sums (one wave x 64 points / x 128 points): each is repeatable bit for bit and held to
 * the reference at the mode's tolerance, but a frame registered alone (k_estep) and the same frame inside a GPU-filling batch (k_estep2) agree
 * to about 1e-8 m, not to the bit.  10: fp64-mode calls repeated without the sigma-following resolution of the E-step's sums because a share was
 * refused under its finer range limits (the repeat runs under the coarse limits of every other mode; only its verdict is reported).
 * 11, 12, 13: always 0 -- these indices belonged to experiments that were measured slower and removed (the spin-ahead loop TDLO_SPIN_AHEAD, a batch's loop
 * in one launch TDLO_BATCH_PERSIST and its repeats; docs/HISTORY.md has the numbers); the indices are not reused.
 * 14: registrations run with one launch per iteration (k_iter_fused, or k_iter_fused_w0 for chains of up to 61 nodes; TDLO_FUSED_W0=0: k_iter_fused for
 * every chain, the comparator); 24 counts those of them whose launches were k_iter_fused_w0.  15 / 16: colour frames (tdlo_colour_depth_to_cloud and the calls built on it) whose
 * segmentation rode in the depth -> cloud launch / that took the mask kernel k_colour_mask (TDLO_COLOUR_FUSED=0, TDLO_CLOUD_FUSED=0, frames passed on).
 * 17: cloud views imported by k_cloud_import (tdlo_set_cloud_view, and the tracker frames that take it).  18: host views that
 * tdlo_tracker_tracking_step_view widened on the host straight into the pinned staging of a small frame.
 * 19 / 20: result images (tdlo_render_result) that k_render wrote where the caller wanted them -- the pinned result buffer, device memory -- / that were
 * copied out of the context's device image (pageable destinations; TDLO_RENDER_INPLACE=0: all of them).
 * 21: tdlo_cloud_view_voxel_grid calls that reached the kernels (tdlo_tracker_frame_from_cloud_view's among them).
 * 22 / 23: tdlo_visibility_prepass calls served by the one-launch kernel k_node_min_dist_direct / by two uploads, k_node_min_dist and a read-back
 * (TDLO_DIRECT_UPLOAD=0); a pre-pass that rode in the depth -> cloud launch is counted by 8 alone.
 * 24: registrations of 14 whose per-iteration launches were k_iter_fused_w0 (recorded where the kernel is chosen).
 * 25 / 26: node sets ordered by k_sort_pts (tdlo_sort_pts, tdlo_tracker_initialize_from_cloud*) / tdlo_tracker_initialize_from_cloud* calls whose
 * centroids were ordered by the host twin (TDLO_INIT_SORT=host).
 * 27 / 28: tdlo_cloud_view_voxel_grid calls (those of tdlo_cloud_view_voxel_grid_visibility and tdlo_tracker_frame_from_cloud_view among them) served by the
 * one-launch kernel / passed on by it to the multi-launch form, a team that gave up included; calls that the host never hands to it (TDLO_CLOUD_FUSED=0,
 * TDLO_CLOUD_TEAM=0, more than 4095 tiles) count in 21 alone.  29: view frames whose visibility pre-pass rode in that launch.  6 / 7 / 8 count depth frames only.
 * 30 / 31: tdlo_visibility_prepass_batch calls served by the one launch k_node_min_dist_batch / passed on to tdlo_visibility_prepass slot by slot.
 * 32 / 33: frames of tdlo_depth_to_cloud_batch (tdlo_tracker_frames_batch's among them) served by the batch launch k_cloud_fused_batch / passed on by it to the
 * single call for their slot; frames of a batch below the crossover, which loops over the single calls, count in 6 / 7 alone.
 * 34 / 35: images of tdlo_render_result_batch (tdlo_tracker_render_result_batch's among them) that k_render_batch wrote where the caller wanted them / that
 * were copied out of the context's arena; 19 / 20 count the single call's images only.
 * 36 / 37: frames of tdlo_reg_batch, tdlo_sort_pts_batch and tdlo_tracker_initialize_from_cloud_batch served by the batch launches (k_reg_estep_batch /
 * k_reg_mstep_batch, k_sort_pts_batch; a frame that ends on TDLO_E_NUMERIC included) / handed to the single call because the batch was smaller than
 * TDLO_INIT_BATCH_MIN; 25 / 26 keep counting the single calls only, those of the second route among them.
 * 38 / 39: frames of tdlo_cloud_view_voxel_grid_batch (tdlo_tracker_frames_from_cloud_view_batch's among them) served by the batch launch k_cloud_view_batch /
 * passed on to the single call for their slot -- by the kernel, or by the host (more than 1 048 576 elements, TDLO_CLOUD_FUSED=0); frames of a batch below
 * the crossover count in 21 / 27 / 28 alone.  40 / 41: frames of tdlo_set_cloud_view_batch (tdlo_tracker_tracking_step_view_batch's among them)
 * imported by the batch launch k_cloud_import_batch / by the single route because the batch was smaller than the crossover.
 * 42 / 43 / 44: frames of tdlo_frame_views_to_cloud_batch (tdlo_tracker_frame_views_batch's among them) served by the batch launches / passed on by the cloud
 * kernel or looped over the single view calls (a batch below the crossover, TDLO_CLOUD_FUSED=0, an image size the one-launch form does not take) / planes
 * written by k_image_import_batch (distinct device views a frame reads; host views are not counted).
 * 45 / 46 / 47: rigs (tdlo_rig_to_cloud, tdlo_rig_to_cloud_visibility, tdlo_tracker_frame_from_rig) served by the one-launch kernel / passed on by it to the
 * multi-launch form (a team that gave up, and the rigs the host never hands to the kernel -- more than 4095 tiles, TDLO_CLOUD_FUSED=0, TDLO_CLOUD_TEAM=0 --
 * included) / whose visibility pre-pass rode in that launch.
 * 48: calls whose prologue was the two launches k_prune_nodes / k_scatter_scan (frames that all prune and sort afresh with one tile per workgroup, at most 256 prune
 * workgroups -- 65 536 points -- and 64 nodes, beyond the fused prologue or with TDLO_DIRECT_UPLOAD=0; TDLO_PROLOGUE_SCAN=0: none, the three-kernel form, the same bits).
 * 49 / 50: frames of tdlo_rig_to_cloud_batch (tdlo_tracker_frames_from_rig_batch's among them) served by the batch launch k_cloud_rig_batch / passed on to
 * tdlo_rig_to_cloud for their slot -- by the kernel (more than 32 704 kept points, too many cell bits, pass-through, the refusals 8 and 9, a result the slot's
 * capacity does not hold), or by the host (more than 4095 tiles, TDLO_CLOUD_FUSED=0); frames of a batch below the crossover count in 45 - 47 alone, and a
 * frame passed on counts there as well.
 * 51 / 52: (camera, frame) jobs of the self-occlusion test under a rig served by k_rig_painter_batch (tdlo_rig_self_occlusion_batch, and the rig tracker calls
 * from kRigPainterMin jobs on) / done by the host statement inside a rig tracker call.
 * 53 / 54: calls of tdlo_cloud_assign, tdlo_cloud_assign_visibility and tdlo_tracker_frames_from_shared_cloud_batch served by the split launches
 * k_assign_count / k_assign_scatter / calls of the latter two in which the pre-pass rode in k_assign_scatter (TDLO_ASSIGN_RIDE=1).
 * 55 / 56: calls of tdlo_cloud_cluster and tdlo_tracker_initialize_from_shared_cloud_batch served by the cluster launches (k_cluster_link and what follows it) /
 * served by the host route (TDLO_CLUSTER=host, or after a lane of k_cluster_link gave up).  A source of 0 points counts in neither.
 * 57 / 58: (camera, cell) jobs of the painter test over a cell of ropes served by k_cell_project / k_cell_cover (tdlo_cell_occlusion_batch, and
 * tdlo_tracker_frames_from_shared_cloud_occluded_batch from kCellPainterMin flat nodes x cameras on) / done by the host statement inside that tracker call.
 * 59 / 60: aligned planes (tdlo_align_depth, and the aligning frame calls) formed by k_align_splat / k_align_pack / by the host statement (TDLO_ALIGN=host).
 * 61 / 62 / 63: jobs of tdlo_align_depth_batch (the aligning rig calls' among them) served by k_align_splat_batch / k_align_pack_batch / by the single launches in
 * a loop (below kAlignBatchMin; these move 59 as well); the distinct jobs formed inside the aligning rig calls.
 * -1 for a null context or an unknown counter. */
long long tdlo_debug_route_count(tdlo_ctx *ctx, int which);
/* Phase stamps (s_memtime) of the last depth -> cloud launch's finishing workgroup; only a -DTDLO_CLOUD_STAMPS build writes them. */
int tdlo_debug_cloud_stamps(tdlo_ctx *ctx, unsigned long long *out, int n);
/* Test aid: provokes a HIP runtime error inside the library (an invalid copy) and reports it like any other: returns TDLO_E_HIP with the
 * text in tdlo_last_error.  The calls that follow must be unaffected -- HIP keeps a per-thread "last error" that the launch checks of a later
 * call would otherwise read (tests/test_parity_gpu.py::test_a_hip_error_does_not_leak_into_the_next_call). */
int tdlo_debug_fail_hip(tdlo_ctx *ctx);
/* Whether the registrations of this context record the four stream events behind tdlo_stats.loop_ms / total_ms.  Off by default: the
 * reference has no such figures, and the markers cost about 15 us per call (2 % of a 50-iteration call at N = 50 000).  Returns the
 * previous setting (or TDLO_E_INVALID). */
int tdlo_set_timing(tdlo_ctx *ctx, int on);
/* Whether registrations of this context may reuse a slot's pruned, node-sorted cloud (see tdlo_cpd_lle_resident).  On by default
 * (off when the environment holds TDLO_REUSE_SORT=0); the reference prunes in every call (trackdlo.cpp:177-195), and a caller that
 * wants every call to pay for that -- a benchmark that registers the same frame again and again -- turns it off.  Returns the
 * previous setting (or TDLO_E_INVALID). */
int tdlo_set_sort_reuse(tdlo_ctx *ctx, int on);
/* The one-shot exchange of tdlo_split_run with ONE rank bound (tdlo_xch_bind, nranks == 1): by default a lone rank has nobody to exchange with and the
 * kernels skip the per-iteration exchange; on != 0: it stores to, flags and reads back its own inbox like any rank of a larger group (what the exchange
 * itself costs on one GPU -- bench.py's self_exchange_iters_per_s; tests).  The same results either way, bit for bit.  Initial value: TDLO_XCH_SELF
 * when the context was made.  Returns the previous setting. */
int tdlo_set_xch_self(tdlo_ctx *ctx, int on);
/* The PCI bus id of the context's GPU ("0000:c1:00.0"; out needs >= 16 bytes): which /sys/bus/pci/devices/<id> node -- clocks, power, busy percentage --
 * belongs to it (bench.py's clock sampler: the container's /sys/class/drm lists every card of the host, not only the visible one). */
int tdlo_pci_bus_id(tdlo_ctx *ctx, char *out, int len);
/* Development aid: copies the pruned, centred, node-sorted cloud of FRAME `frame` OF THE LAST CALL (N x 3 column-major, widened to
 * double) and that frame's centring offset; returns N.  The last call's frame list has one entry per frame of that call: frame i of a
 * tdlo_cpd_lle_batch, and exactly frame 0 of a single registration whatever slot it ran on.  TDLO_E_INVALID beyond the list (or N > max_points). */
int tdlo_debug_read_cloud(tdlo_ctx *ctx, int frame, double *out, int max_points, double *ctr);
/* Development aid: what the set-up stage (prune / sort / centring / chain links) left in device memory for frame `frame` of the last call
 * (frames counted as for tdlo_debug_read_cloud), copied to out (capacity cap doubles); returns the number of doubles, or TDLO_E_INVALID.
 *   TDLO_SETUP_COORD   M       the chain coordinate (trackdlo.cpp:214-223)
 *   TDLO_SETUP_CHAIN   8 M     row 0 {Pinf11, Pinf22, 1/Pinf11, 1/Pinf22, 0 ...}, row i {Phi11, Phi12, Phi21, Phi22, Q11, Q12, Q22, 0} of the gap (i - 1, i)
 *   TDLO_SETUP_HY0     3 M     H Y0, column-major (registrations with the LLE term only: TDLO_E_INVALID otherwise)
 *   TDLO_SETUP_Y0      3 M     the incoming nodes less the centring offset, fp64, column-major
 *   TDLO_SETUP_NODES   4 M     the node block of the E-step {x, y, z, coord} in compute precision, widened: x, y, z are the CURRENT nodes -- the
 *                              incoming ones only until the first M-step has run (after tdlo_split_begin, say); coord stays
 *   TDLO_SETUP_KEEP    4       {kept points, sum of d2} as kept with the slot's sorted cloud (not written by tdlo_split_begin), then the same two
 *                              numbers from the registration's state
 *   TDLO_SETUP_SIGMA2  1       the state's sigma2 as it stands: every M-step overwrites it, so it is the iteration-0 value only before the first
 *                              one (after tdlo_split_begin + tdlo_split_set_global); elsewhere sigma2_0 = sum / (3 M kept) from TDLO_SETUP_KEEP */
#define TDLO_SETUP_COORD 0
#define TDLO_SETUP_CHAIN 1
#define TDLO_SETUP_HY0 2
#define TDLO_SETUP_Y0 3
#define TDLO_SETUP_NODES 4
#define TDLO_SETUP_KEEP 5
#define TDLO_SETUP_SIGMA2 6
int tdlo_debug_read_setup(tdlo_ctx *ctx, int frame, int what, double *out, int cap);

#ifdef __cplusplus
}
#endif
#endif
