// tdlo_api.cpp -- C ABI (include/trackdlo_hip.h): context, frame slots, the cpd_lle driver, the
// batched and N-split forms, and the tracker object mirroring class trackdlo
// (trackdlo/include/trackdlo.h:53-130, trackdlo/src/trackdlo.cpp:8-90, :900-999).
#include "../../include/trackdlo_hip.h"
#include "tdlo_internal.h"
#include "tdlo_host.h"
#include "tdlo_image.h"
#include "tdlo_rccl.h"
#include "tdlo_reg_plan.h"
#include "tdlo_rig_host.h"
#include "tdlo_painter_host.h"
#include "tdlo_cell_painter_host.h"
#include "tdlo_assign_host.h"
#include "tdlo_cluster_lane.h"
#include "tdlo_align_host.h"
#include "tdlo_align_batch_plan.h"
#include "tdlo_view_batch_plan.h"
#include "tdlo_rig_batch_plan.h"

#include <algorithm>
#include <limits>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace tdlo;

namespace {

#define TDLO_RET(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

constexpr int kMaxEstepBlocks = 4096;      // (upper bound of TDLO_ESTEP_BLOCKS / tdlo_config.estep_blocks; the defaults are 512 and 1024)
constexpr int kBatchStreams = 4;       // streams a batch of frames is spread over (run_frames); more than 4 lose (measured: 6 or 8 fall below one stream)
constexpr int kIterHintMax = 8;        // tdlo_ctx::iter_hint: at most this many iterations go out before the host first looks
constexpr int kEstepWideMin = 129;          // (measured: scripts/gpu_estep_wide_ab.py)
constexpr int kEstep2MinWaves = 2048;   // 64-point batches of a cloud (or of a batch's frames together) from which the E-step is k_estep2 (two points per lane): two waves per SIMD
constexpr int kChunkIters = 4;          // EM iterations per early-exit polling chunk; the first chunks are shorter (1, 1, 2):
                                        // a tracker in steady state converges in one or two iterations

struct Slot {
    // cloud-sized
    int cap_points = 0;
    int N0 = 0;
    double *Xraw = nullptr;
    void *Xs = nullptr;
    unsigned short *bucket = nullptr;
    int *hist = nullptr;
    size_t hist_ints = 0;
    double *blksum = nullptr;
    // what the sorted cloud Xs was last made for (prune + counting sort by nearest node depend on the cloud and on the nodes only): a
    // registration of the SAME nodes on the same cloud in the same precision reuses it (FrameDev::reuse_sorted)
    std::vector<double> sorted_Y;
    int sorted_prec = -1;
    bool sorted_valid = false;
    // node-sized (one allocation, carved)
    int cap_nodes = 0;
    double *nodeblk = nullptr;
    size_t nodeblk_doubles = 0;
    unsigned *sync = nullptr;        // 256 words, zeroed once: cross-workgroup hand-off state of the multi-CU M-step
    unsigned fuse_epoch = 0;         // launches of the fused prologue on this slot (its grid barrier's flag carries the number)
    // a second node block: tracking_step with every node visible has the fused prologue of its first registration set up the second one as
    // well (PairNext) -- the second registration then runs out of this block
    int cap_nodes2 = 0;
    double *nodeblk2 = nullptr;
    // the LLE regulariser (13 diagonals) of the nodes the last tracking_step left behind, formed on the device by the M-step that finished its
    // main registration (FrameDev::lle_next): serves the next pre-processing registration if it starts from exactly those nodes
    double *hb_next = nullptr;
    int hb_next_cap = 0;
    std::vector<double> hb_next_Y;
    bool hb_next_valid = false;
};

struct NodeCarve {
    // offsets in doubles into Slot::nodeblk for a given M; the first `upload` doubles are the
    // host-supplied block [descriptor | Yin | aJ | aYd | Hb | H]: without the LLE term it ends in front of Hb, with the banded LLE M-step in
    // front of H (Hb = the 13 diagonals of H, 13 M doubles instead of M^2), with the dense LLE M-steps it is the whole block; [Yout | IterState]
    // comes back.
    size_t fdev, Yin, aJ, aYd, Hb, H, upload;      // fdev: the frame's descriptor travels at the head of the upload block (one frame per call)
    size_t Yout, st, readback;
    size_t ctr, Y, Y0, nodes, coord, G, chain, HG, HY0, dmin, sums, dbg, Ascr, acc, band, total;
    size_t Yout2, st2, Y2, nodes2;                 // the second copies of result, state, Y and nodes of the loop with one launch per iteration (tdlo_iter_fused.hip)
    explicit NodeCarve(int M) {
        const size_t m = (size_t)M, mm = m * m;
        size_t o = 0;
        auto take = [&](size_t n) { size_t r = o; o += (n + 1) & ~(size_t)1; return r; };   // keep 16-byte alignment
        fdev = take((sizeof(FrameDev) + 7) / 8);
        Yin = take(3 * m); aJ = take(m); aYd = take(3 * m); Hb = take(13 * m); H = take(mm); upload = o;
        Yout = take(3 * m); st = take((sizeof(IterState) + 7) / 8); readback = o - Yout;
        ctr = take(4); Y = take(3 * m); Y0 = take(3 * m); nodes = take(4 * m); coord = take(m);
        G = take(mm); chain = take(8 * (m + 1)); HG = take(mm); HY0 = take(3 * m); dmin = take(m); sums = take(4 * m + 2); dbg = take(64);
        Ascr = take(std::max((size_t)(M | 1) * (m + 3), mstep_big_scratch_doubles(M)));
        acc = take((size_t)3 * kAccRows * (4 * m + 2));       // the E-step's fixed-point accumulators: two iteration parities; the loop with one launch per iteration
                                                              // (tdlo_iter_fused.hip) rotates over three buffers
        band = take(band_record_doubles(M));                  // column records of the banded LLE M-step
        Yout2 = take(3 * m); st2 = take((sizeof(IterState) + 7) / 8);      // ([Yout | IterState] laid out as the read-back block is: host_publish)
        Y2 = take(3 * m); nodes2 = take(4 * m);
        total = o;
    }
};

}  // namespace

// Host threads that enqueue the stream groups of a batch side by side.  A 32-frame call is 400 kernel launches of ~4 us of host time
// each -- as long as the GPU needs to run them -- so one enqueueing thread makes the batch host-bound whenever the CPU is a little
// slower than usual (measured: 0.86 ... 1.03 M it/s run to run); every group's launches go to its own stream anyway.
struct EnqueuePool {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv, cv_done;
    std::function<int(int)> job;
    int gen = 0, pending = 0, first_err = 0, device = 0;
    bool stop = false;
    void start(int n, int dev) {
        device = dev;
        for (int i = 0; i < n; ++i) th.emplace_back([this, i] { loop(i + 1); });
    }
    void loop(int idx) {
        (void)hipSetDevice(device);
        int seen = 0;
        for (;;) {
            std::function<int(int)> f;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return stop || gen != seen; });
                if (stop) return;
                seen = gen; f = job;
            }
            const int rc = f(idx);
            {
                std::lock_guard<std::mutex> lk(m);
                if (rc && !first_err) first_err = rc;
                if (--pending == 0) cv_done.notify_one();
            }
        }
    }
    // f(1) .. f(th.size()) on the workers, f(0) on the caller; returns the first non-zero result
    int run(const std::function<int(int)> &f) {
        {
            std::lock_guard<std::mutex> lk(m);
            job = f; pending = (int)th.size(); first_err = 0; ++gen;
        }
        cv.notify_all();
        const int rc0 = f(0);
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return pending == 0; });
        return rc0 ? rc0 : first_err;
    }
    ~EnqueuePool() {
        { std::lock_guard<std::mutex> lk(m); stop = true; }
        cv.notify_all();
        for (auto &t : th) t.join();
    }
};

struct tdlo_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    double *xfer = nullptr;          // batches: device mirror of [F upload blocks | F read-back blocks], moved with one copy each way
    size_t xfer_doubles = 0;
    hipStream_t stream2[kBatchStreams - 1] = {};   // further groups of a batch: their E-steps overlap another group's one-workgroup-per-frame M-step
    hipEvent_t evx[kBatchStreams] = {}, evj[kBatchStreams] = {};   // fork / join of the batch groups
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // 0..3 timing, 4..5 early-exit polling
    tdlo_config cfg{};
    std::vector<Slot> slots;
    std::vector<FrameDev> fh;        // host copies of the frame descriptors of the last call
    FrameDev *fd = nullptr;          // device array [max_frames]
    double *pin = nullptr;           // pinned staging
    double *reg_ws = nullptr;        // `reg` workspace
    size_t reg_ws_cap = 0;
    void *cloud_ws = nullptr;        // depth -> cloud workspace (images, sort buffers)
    size_t cloud_ws_cap = 0;
    // depth -> cloud in one launch (k_cloud_fused): its own workspace behind the same images, the pinned words the kernel reports through, and the
    // pinned image buffers a caller may fill directly (tdlo_image_buffers: the kernel then reads the images over PCIe, no copy).  TDLO_CLOUD_FUSED=0:
    // the multi-launch form (comparator)
    void *cloud_fws = nullptr;
    size_t cloud_fws_cap = 0;
    bool cloud_fused_first = true;   // the kernel's state words have to be initialised (first launch, after a failed one, after a reallocation)
    unsigned long long *cloud_res = nullptr;
    unsigned cloud_epoch = 0;
    char *img_pin = nullptr;
    size_t img_pin_cap = 0;
    int img_pin_rows = 0, img_pin_cols = 0;
    bool cloud_fused_on = !(getenv("TDLO_CLOUD_FUSED") && atoi(getenv("TDLO_CLOUD_FUSED")) == 0);
    bool cloud_team_on = !(getenv("TDLO_CLOUD_TEAM") && atoi(getenv("TDLO_CLOUD_TEAM")) == 0);      // 0: ONE finishing workgroup (k_cloud_fused) instead of the last eight as a team (k_cloud_team)
    // visibility pre-pass in one launch (k_node_min_dist_direct): minima + ticket on the device (kept armed by the kernel), [word | M minima] in pinned host memory
    unsigned long long *vis_state = nullptr, *vis_res = nullptr;
    unsigned vis_epoch = 0;
    bool vis_armed = false;
    double *vis_nodes_pin = nullptr;     // 3 x 64 doubles in pinned host memory: the nodes of a pre-pass that rides in the depth -> cloud team kernel
    long long cloud_vis_rides = 0;       // how many frames' pre-passes did (tdlo_debug_route_count 8)
    // tdlo_tracker_initialize_from_cloud: TDLO_INIT_SORT=host orders reg's centroids with the host twin (sort_pts_host) after reading them back -- the comparator,
    // the same bits; init_route: tdlo_debug_route_count 25 / 26 -- calls ordered by k_sort_pts (tdlo_sort_pts among them) / by the host twin
    bool init_sort_host = getenv("TDLO_INIT_SORT") && getenv("TDLO_INIT_SORT")[0] == 'h';
    long long init_route[2] = {0, 0};
    // tdlo_reg_batch / tdlo_sort_pts_batch / tdlo_tracker_initialize_from_cloud_batch: from init_batch_min frames on the frames share the launches
    // (tdlo_reg_batch.hip, k_sort_pts_batch), below it the call loops over the single calls (kInitBatchMin = 1: never, unless TDLO_INIT_BATCH_MIN=n, read here, says so).
    // ibat_route: tdlo_debug_route_count 36 / 37 -- frames served by the batch launches / handed to the single call
    int init_batch_min = (getenv("TDLO_INIT_BATCH_MIN") && atoi(getenv("TDLO_INIT_BATCH_MIN")) >= 1) ? atoi(getenv("TDLO_INIT_BATCH_MIN")) : 0;      // 0: kInitBatchMin
    long long ibat_route[2] = {0, 0};
    // the pre-pass of F slots in one launch (k_node_min_dist_batch, tdlo_batch.hip): a state of its own -- [vbat_cap minima | ticket], grown on demand and armed
    // when allocated, kept armed by the kernel -- and [word | F M minima] in pinned host memory
    unsigned long long *vbat_state = nullptr, *vbat_res = nullptr;
    size_t vbat_cap = 0;
    unsigned vbat_epoch = 0;
    bool vbat_armed = false;
    long long vbat_route[2] = {0, 0};    // tdlo_debug_route_count 30 / 31: tdlo_visibility_prepass_batch calls served by the one launch / passed on to tdlo_visibility_prepass per slot
    long long vis_route[2] = {0, 0};     // tdlo_debug_route_count 22 / 23: tdlo_visibility_prepass calls served by the one-launch kernel / by the copies + k_node_min_dist
    long long cloud_route[2] = {0, 0};   // tdlo_debug_route_count 6 / 7: depth -> cloud calls served by the one-launch kernel / sent on to the multi-launch form by it
    // clouds for F slots in one call (tdlo_depth_to_cloud_batch, k_cloud_fused_batch): the arena -- cbat_dev: the frame blocks (tile regions, state words,
    // workspace; frame f's at f x cloud_batch_frame_bytes(P) whatever F is), cbat_img: [descriptor table | image planes] -- in device memory and
    // [2 F result words | descriptor table] in pinned host memory, all grown on demand; the first cbat_armed_F frame blocks' state words are armed for images
    // of cbat_armed_P pixels (the kernel keeps them so; a call that did not complete, another size or a reallocation has them initialised again)
    void *cbat_dev = nullptr, *cbat_img = nullptr;
    size_t cbat_dev_cap = 0, cbat_img_cap = 0;
    char *cbat_pin = nullptr;
    size_t cbat_pin_cap = 0;
    int cbat_armed_F = 0, cbat_armed_P = 0;
    int cloud_batch_min = (getenv("TDLO_CLOUD_BATCH_MIN") && atoi(getenv("TDLO_CLOUD_BATCH_MIN")) >= 1) ? atoi(getenv("TDLO_CLOUD_BATCH_MIN")) : 0;      // 0: kCloudBatchMin
    long long cbat_route[2] = {0, 0};    // tdlo_debug_route_count 32 / 33: frames served by the batch launch / passed on by it to the single call
    // image views for F slots in one call (tdlo_frame_views_to_cloud_batch: k_image_import_batch into the same arena, then k_cloud_fused_batch).  Behind the
    // descriptor table the arena holds the import's job table, in pinned memory behind both the host views' canonical planes as their arena region has them
    // (one copy brings tables and planes up).  fvbat_planes: per image of the most recent view batch the arena addresses of its canonical planes by role
    // (depth, colour, occluder, mask; nullptr: not imported) -- tdlo_view_batch_images; emptied by whatever writes the arena next.
    // TDLO_FRAME_VIEW_BATCH_MIN=n: below n frames the calls loop over the single view calls (0: kFrameViewBatchMin / kFrameViewBatchTrackerMin).
    // fvbat_route: tdlo_debug_route_count 42 / 43 / 44 -- frames served by the batch launches / passed on or looped / planes k_image_import_batch wrote
    struct ViewBatchPlanes { const void *p[4]; };
    std::vector<ViewBatchPlanes> fvbat_planes;
    int frame_view_batch_min = (getenv("TDLO_FRAME_VIEW_BATCH_MIN") && atoi(getenv("TDLO_FRAME_VIEW_BATCH_MIN")) >= 1) ? atoi(getenv("TDLO_FRAME_VIEW_BATCH_MIN")) : 0;
    long long fvbat_route[3] = {0, 0, 0};
    // cloud views for F slots in one call (tdlo_cloud_view_voxel_grid_batch: k_cloud_view_batch; tdlo_set_cloud_view_batch: k_cloud_import_batch).  wbat_dev: the
    // arena of tdlo_view_batch_plan.h -- [one state block per slot of the context | descriptor table | the frames' blocks] -- grown on demand; the state blocks
    // are armed when wbat_armed says so (the kernel keeps them so; a call that did not complete or a reallocation has them initialised again).  wbat_pin:
    // [2 F result words | the table as it is uploaded | the host views packed column-major in their own precision, every distinct view once | the host
    // selection bytes], read in place by the kernels.  wbat_ev: one event per distinct ready_stream of a call.  TDLO_VIEW_BATCH_MIN=n: below n frames the
    // calls loop over the single calls (0: kViewBatchMin / kViewBatchTrackerMin).  wbat_route: tdlo_debug_route_count 38 .. 41
    void *wbat_dev = nullptr;
    size_t wbat_dev_cap = 0;
    char *wbat_pin = nullptr;
    size_t wbat_pin_cap = 0;
    bool wbat_armed = false;
    std::vector<hipEvent_t> wbat_ev;
    int view_batch_min = (getenv("TDLO_VIEW_BATCH_MIN") && atoi(getenv("TDLO_VIEW_BATCH_MIN")) >= 1) ? atoi(getenv("TDLO_VIEW_BATCH_MIN")) : 0;
    long long wbat_route[4] = {0, 0, 0, 0};
    long long rig_route[3] = {0, 0, 0};         // tdlo_debug_route_count 45 / 46 / 47: rigs (tdlo_rig_to_cloud) served by the one-launch kernel / passed on by it / whose pre-pass rode in it
    // rigs for F slots in one call (tdlo_rig_to_cloud_batch: k_cloud_rig_batch).  rbatch_dev: the arena of tdlo_rig_batch_plan.h -- [one state block per slot of
    // the context | frame table | camera table | every distinct plane once | the frame blocks of one launch] -- grown on demand; the state blocks are armed when
    // rbatch_armed says so (the kernel keeps them so; a call that did not complete or a reallocation has them initialised again).  rbatch_pin: [result words |
    // frame table | camera table].  TDLO_RIG_BATCH_MIN=n: below n frames the calls loop over the single calls (0: kRigBatchMin / kRigBatchTrackerMin).
    // rbatch_route: tdlo_debug_route_count 49 / 50: frames the batch launch served / frames passed on to the single call
    void *rbatch_dev = nullptr;
    size_t rbatch_dev_cap = 0;
    char *rbatch_pin = nullptr;
    size_t rbatch_pin_cap = 0;
    bool rbatch_armed = false;
    int rig_batch_min = (getenv("TDLO_RIG_BATCH_MIN") && atoi(getenv("TDLO_RIG_BATCH_MIN")) >= 1) ? atoi(getenv("TDLO_RIG_BATCH_MIN")) : 0;
    long long rbatch_route[2] = {0, 0};
    // the self-occlusion test under a rig (tdlo_rig_self_occlusion_batch: k_rig_painter_batch).  pnt_pin: [frame table | camera records | nodes | result words]
    // in pinned host memory -- the first three go up in ONE copy into pnt_dev, the kernel stores the words where they lie --, both grown on demand.
    // TDLO_RIG_PAINTER_MIN=n: tracker calls with fewer than n (camera, frame) jobs run the host statement (0: kRigPainterMin).
    // pnt_route: tdlo_debug_route_count 51 / 52: jobs served by the kernel / done by the host statement
    void *pnt_dev = nullptr;
    size_t pnt_dev_cap = 0;
    char *pnt_pin = nullptr;
    size_t pnt_pin_cap = 0;
    int rig_painter_min = (getenv("TDLO_RIG_PAINTER_MIN") && atoi(getenv("TDLO_RIG_PAINTER_MIN")) >= 1) ? atoi(getenv("TDLO_RIG_PAINTER_MIN")) : 0;
    long long pnt_route[2] = {0, 0};
    // the painter test over a cell of ropes (tdlo_cell_occlusion_batch: k_cell_project / k_cell_cover).  cel_pin: [cell table | camera records | nodes | link
    // words | result words] in pinned host memory -- all but the last go up in ONE copy into cel_dev, whose tail holds the kernels' (camera, cell) tables --,
    // both grown on demand.  TDLO_CELL_PAINTER_MIN=n: the tracker call runs the host statement on a cell of fewer than n flat nodes x cameras (0: always the kernels).
    // cel_route: tdlo_debug_route_count 57 / 58: jobs served by the kernels / done by the host statement
    void *cel_dev = nullptr;
    size_t cel_dev_cap = 0;
    char *cel_pin = nullptr;
    size_t cel_pin_cap = 0;
    long long cell_painter_min = (getenv("TDLO_CELL_PAINTER_MIN") && *getenv("TDLO_CELL_PAINTER_MIN") && atoll(getenv("TDLO_CELL_PAINTER_MIN")) >= 0)
                                     ? atoll(getenv("TDLO_CELL_PAINTER_MIN")) : -1;      // (-1: not set)
    long long cel_route[2] = {0, 0};
    // one cloud dealt out among F slots (tdlo_cloud_assign and the calls built on it: k_assign_count / k_assign_scatter).  asg_dev: [table | owner | g | counts]
    // in device memory, grown on demand; asg_state: [asg_state_cap minima | ticket], armed when allocated or after a launch that did not report, kept armed by
    // the kernel; asg_res: [word | F counts | T minima] in pinned host memory.  TDLO_ASSIGN_RIDE=1: the pre-pass rides in k_assign_scatter (measured slower, profiles/cloud_assign_ab.txt: off by default).
    // asg_route: tdlo_debug_route_count 53 / 54: calls the split launches served / calls in which the pre-pass rode
    char *asg_dev = nullptr;
    size_t asg_dev_cap = 0;
    unsigned long long *asg_state = nullptr, *asg_res = nullptr;
    size_t asg_state_cap = 0, asg_res_cap = 0;
    unsigned asg_epoch = 0;
    bool asg_armed = false;
    bool assign_ride = getenv("TDLO_ASSIGN_RIDE") && atoi(getenv("TDLO_ASSIGN_RIDE")) != 0;
    long long asg_route[2] = {0, 0};
    // one cloud clustered into ropes (tdlo_cloud_cluster and the tracker call built on it: tdlo_cluster.hip in front of k_assign_scatter).  Its workspace (parent,
    // size, rank, the kept-root counts) lies in asg_dev behind the split's own blocks; asg_res carries two more words (give-up, C).  TDLO_CLUSTER=host: the owners
    // come from the host statement.  clu_route: tdlo_debug_route_count 55 / 56: calls the cluster launches served / calls the host route served (forced, or after a give-up)
    bool cluster_host = getenv("TDLO_CLUSTER") && std::strcmp(getenv("TDLO_CLUSTER"), "host") == 0;
    long long clu_route[2] = {0, 0};
    // depth aligned to the colour camera (tdlo_align_depth and the aligning frame calls: k_align_splat / k_align_pack).  aln_dev: [scratch plane of 32-bit words |
    // aligned uint16 plane | packed depth of a host view | 4 count words], grown on demand; the scratch words and the counts are armed (all ones / zero) when
    // allocated or after a call that failed between its launches, and kept armed by k_align_pack.  aln_res: 4 count words in pinned host memory; aln_pin: the
    // pinned staging of a host view's packed depth (and of the host route's plane).  TDLO_ALIGN=host: the plane comes from the host statement and is uploaded
    // (the comparator).  aln_route: tdlo_debug_route_count 59 / 60: planes formed by the kernels / by the host statement
    char *aln_dev = nullptr, *aln_pin = nullptr;
    size_t aln_dev_cap = 0, aln_pin_cap = 0, aln_Pc = 0, aln_Pd = 0;
    unsigned long long *aln_res = nullptr;
    bool aln_armed = false;
    int aln_res_at = 0;                   // where in aln_res the last call's counts lie: 0 (written by k_align_pack) or 4 (the host route's)
    bool align_host = getenv("TDLO_ALIGN") && std::strcmp(getenv("TDLO_ALIGN"), "host") == 0;
    long long aln_route[5] = {0, 0, 0, 0, 0};
    // ... for many cameras in one call (tdlo_align_depth_batch and the aligning rig calls: k_align_splat_batch / k_align_pack_batch).  alnb_dev: the arena of
    // tdlo_align_batch_plan.h, [scratch region | uint16 planes | count words | job table], grown on demand; alnb_armed: the bytes of the scratch region filled with
    // all ones and kept so by k_align_pack_batch (the header's invariant).  alnb_up: the packed depth of the call's host views in device memory.  alnb_pin: pinned,
    // [4 x 1024 count words the pack kernel writes | zeroed count words and the job table, copied up in one piece | the host views' packed depth, one copy (the host
    // route: its depth images and planes)].  alnb_ev_up: recorded behind a call's uploads -- the next call waits for it before it writes alnb_pin again.  alnb_ev: one
    // event per distinct ready_stream of a call.  alnb_host_counts: the host route's counts.  aln_route[2 ..]: tdlo_debug_route_count 61 / 62 / 63: jobs the batch
    // launches served / jobs the single launches served in a loop / distinct jobs formed inside the aligning rig calls
    char *alnb_dev = nullptr, *alnb_up = nullptr, *alnb_pin = nullptr;
    size_t alnb_cap = 0, alnb_armed = 0, alnb_up_cap = 0, alnb_pin_cap = 0;
    hipEvent_t alnb_ev_up = nullptr;
    bool alnb_up_pending = false;
    std::vector<hipEvent_t> alnb_ev;
    std::vector<long long> alnb_host_counts;
    int align_batch_min = (getenv("TDLO_ALIGN_BATCH_MIN") && atoi(getenv("TDLO_ALIGN_BATCH_MIN")) >= 1) ? atoi(getenv("TDLO_ALIGN_BATCH_MIN")) : 0;
    long long view_team_route[3] = {0, 0, 0};   // tdlo_debug_route_count 27 / 28 / 29: voxel-grid view calls served by the one-launch kernel / passed on by it / whose pre-pass rode in it
    // colour segmentation in front of depth -> cloud (tdlo_colour_*): pinned colour + occluder images a caller may fill directly (tdlo_colour_buffers: read in
    // place over PCIe), the device copies of images handed over elsewhere (colour | occluder | HSV image of tdlo_colour_mask).  TDLO_COLOUR_FUSED=0: the mask
    // kernel (k_colour_mask), then the mask route as it is without colour (comparator)
    char *col_pin = nullptr;
    size_t col_pin_cap = 0;
    int col_pin_rows = 0, col_pin_cols = 0;
    void *col_dev = nullptr;
    size_t col_dev_cap = 0;
    bool colour_fused_on = !(getenv("TDLO_COLOUR_FUSED") && atoi(getenv("TDLO_COLOUR_FUSED")) == 0);
    long long colour_route[2] = {0, 0};  // tdlo_debug_route_count 15 / 16: frames whose segmentation rode in the depth -> cloud launch / that took the mask kernel
    // the tracking-result image (tdlo_render_result, k_render).  last_*: where the most recent colour call left its colour and occluder images for the
    // device (colour_stage: the device copies, or the pinned buffers) -- what a render call without images of its own draws over.  res_pin: the pinned
    // result image a caller may ask for (tdlo_result_image_buffer); res_dev: the device image that is copied out for any other destination; rnd_pin /
    // rnd_dev: [primitive table | the two corner words], staged and resident.  TDLO_RENDER_INPLACE=0: the kernel never writes the caller's memory
    // itself -- always res_dev and a copy (the comparator; profiles/render_frame_ab.txt).  render_route: tdlo_debug_route_count 19 / 20
    const unsigned char *last_colour = nullptr, *last_occluder = nullptr;
    // where the last view call (tdlo_frame_to_cloud_view and its kin) left the frame's canonical images, by role (depth, colour, occluder, mask): the device
    // buffers or the pinned ones; nullptr: the frame had no such image (tdlo_debug_read_images)
    const void *view_img[4] = {nullptr, nullptr, nullptr, nullptr};
    int view_rows = 0, view_cols = 0;
    int last_col_rows = 0, last_col_cols = 0;
    char *res_pin = nullptr;
    size_t res_pin_cap = 0;
    int res_pin_rows = 0, res_pin_cols = 0;
    void *res_dev = nullptr;
    size_t res_dev_cap = 0;
    char *rnd_pin = nullptr, *rnd_dev = nullptr;
    bool render_inplace = !(getenv("TDLO_RENDER_INPLACE") && atoi(getenv("TDLO_RENDER_INPLACE")) == 0);
    long long render_route[2] = {0, 0};  // images the kernel wrote where the caller wanted them / images copied out of res_dev
    // result images for many ropes and images in one launch (tdlo_render_result_batch, k_render_batch): rbat_dev = [image records | rope heads | primitive
    // records | corner words | staged sources | images to be copied out] in device memory, rbat_pin = [the table as it is uploaded | the corner words as they
    // are read back] in pinned host memory, both grown on demand.  rbat_route: tdlo_debug_route_count 34 / 35
    char *rbat_dev = nullptr, *rbat_pin = nullptr;
    size_t rbat_dev_cap = 0, rbat_pin_cap = 0;
    long long rbat_route[2] = {0, 0};    // images k_render_batch wrote where the caller wanted them / images copied out of rbat_dev
    size_t pin_doubles = 0;
    std::string err;
    int last_F = 0;
    bool lle_batch_dense = false;         // run_frames: a frame of this batch cannot take the banded LLE solve, all of them are staged for the dense kernels
    bool lle_dense_once = false;          // run_frames' retry: the banded LLE solve reported a numeric failure, this call repeats with the dense pivoted kernels
    long long band_retries = 0;           // how often that happened (tdlo_debug_band_retries)
    long long route_count[6] = {0, 0, 0, 0, 0, 0};   // tdlo_debug_route_count: 0 paired set-ups taken up, 1 first iterations started from the handed-over sums,
                                               // 2 M-steps released from their wait for priors, 3 pre-processing registrations served by a device-formed H,
                                               // 4 main registrations whose first iteration ran beside the pre-processing registration (PairNext::ahead),
                                               // 5 calls repeated on the three-kernel route because the fused prologue's grid barrier was abandoned (fuse_fallback)
    // The fused prologue (k_prologue) needs all its workgroups resident at once; its grid barrier gives up after 2 s (tdlo_device.hip, fuse_wait) and
    // the registration then ends with TDLO_E_FUSE: the call is repeated on the copy + three-kernel route and this context stops using the fused
    // prologue (a GPU that could not co-schedule <= 66 workgroups once -- masked or partitioned CUs, long-running kernels of other processes -- is
    // not asked again; every wait costs the caller 2 s).  TDLO_FUSE_FORCE_TIMEOUT=n (test hook): the context's n-th fused launch withholds one arrival.
    bool fuse_on = true;
    int fuse_force_timeout = getenv("TDLO_FUSE_FORCE_TIMEOUT") ? atoi(getenv("TDLO_FUSE_FORCE_TIMEOUT")) : 0;
    bool sort_reuse = !(getenv("TDLO_REUSE_SORT") && atoi(getenv("TDLO_REUSE_SORT")) == 0);   // tdlo_set_sort_reuse: a slot's sorted cloud may serve the next registration of the same nodes
    // results mailbox in pinned host memory (FrameDev::host_out / host_prog): [read-back block | progress word], written by the one-workgroup M-steps
    double *mbox = nullptr;
    size_t mbox_doubles = 0;
    unsigned mbox_epoch = 0;
    // TDLO_PROLOGUE_SCAN=0: clouds beyond the fused prologue keep k_prune_pass1 / k_setup / k_prune_scatter (the comparator of the two-launch
    // prologue k_prune_nodes / k_scatter_scan, launch_prologue_scan; the same bits)
    bool prologue_scan_on = !(getenv("TDLO_PROLOGUE_SCAN") && atoi(getenv("TDLO_PROLOGUE_SCAN")) == 0);
    long long prologue_scan_calls = 0;    // calls whose prologue was those two launches, as launch_prologue_scan reports them (tdlo_debug_route_count 48)
    bool direct_in = !(getenv("TDLO_DIRECT_UPLOAD") && atoi(getenv("TDLO_DIRECT_UPLOAD")) == 0);   // one frame per call: the set-up kernels read the host-supplied block from pinned host
                                                                                                // memory themselves (small clouds: the fused prologue); 0: copy + three launches (comparator)
    double *late_buf = nullptr;           // pinned: [alpha J | alpha (Y_ext - Y0)] of priors that arrive after the set-up kernel was launched (FrameDev::late_aJ)
    size_t late_doubles = 0;
    bool late_on = !(getenv("TDLO_LATE_PRIORS") && atoi(getenv("TDLO_LATE_PRIORS")) == 0);   // tracking_step: priors formed beside the second registration's set-up kernel; 0: before it (comparator)
    bool mbox_on = !(getenv("TDLO_HOST_MAILBOX") && atoi(getenv("TDLO_HOST_MAILBOX")) == 0);   // TDLO_HOST_MAILBOX=0: the read-back copy + stream wait of rounds 1-3 (comparator)
    // tracking_step, every node visible: both registrations start from the SAME nodes on the same cloud, and the second one's node-side set-up
    // (centring, chain links, iteration constants: k_setup's work) depends on nothing the first one produces.  The first registration's fused
    // prologue then runs it as one more workgroup beside its own (k_prologue, blockIdx = nb + 1) into the slot's second node block, and the
    // second registration starts at its E-step: one launch and one dependent-dispatch gap less per frame.  TDLO_PAIR_SETUP=0: off (comparator).
    struct PairNext {
        int state = 0;                    // 0: nothing; 1: asked for by tracking_step (inputs below); 2: set up on the device (f, up)
        int slot = 0, M = 0, n_vis = 0;
        double sigma2 = 0;
        tdlo_params p{};
        std::vector<double> Y;
        FrameDev f{};
        size_t up = 0;
        bool has_sums = false;            // the pre-processing registration's first M-step leaves the first E-step's sums for it (FrameDev::pair_sums)
        // tracking_step with HIDDEN nodes: the two registrations start from different node sets, so nothing is shared -- but the main registration's
        // prologue (prune, sort, set-up), k_dmin and first E-step depend on nothing the pre-processing registration produces either.  state 3 = asked
        // for by tracking_step: the pre-processing registration's run_frames, once its own first iterations are on the stream, launches them on a
        // SECOND stream into the context's twin slot (own cloud buffers, own node block; the cloud is read from the same pinned staging buffer), with
        // the first M-step behind them waiting for the priors (FrameDev::spec_flag, spec_prev == nullptr; FrameDev::late_mstep).  They run beside the
        // pre-processing registration's 6-7 iterations; the main registration (state 2, ahead) then only releases that M-step and stays on the second
        // stream.  TDLO_AHEAD=0: off (comparator).
        bool ahead = false;
        bool cloud_in_pin = false;        // (request) this frame's cloud is in tdlo_ctx::cloud_pin
        int spec = 0;                     // 1: its first M-step is already on the stream, waiting for the priors (FrameDev::spec_flag)
        unsigned spec_epoch = 0;          // ... under this mailbox epoch
    } pair;
    double *pin2 = nullptr;               // pinned: the paired registration's upload block
    size_t pin2_doubles = 0;
    bool pair_on = !(getenv("TDLO_PAIR_SETUP") && atoi(getenv("TDLO_PAIR_SETUP")) == 0);
    Slot twin;                            // PairNext::ahead: the main registration's cloud buffers and node block while it runs beside the pre-processing one
    bool twin_busy = false;               // something launched ahead into the twin slot may still be running on the second stream (drained before its staging block is reused)
    bool ahead_on = !(getenv("TDLO_AHEAD") && atoi(getenv("TDLO_AHEAD")) == 0);
    // tracking_step: the frame's cloud staged in pinned host memory and read from there by the fused prologue's point workgroups (FrameDev::Xhost)
    // instead of a host-to-device copy in front of it (a 9 us copy on the stream, 8 us of host time for the call); cloud_pending: staged for this
    // slot and not yet on the device.  TDLO_DIRECT_CLOUD=0: the copy (comparator)
    double *cloud_pin = nullptr;
    size_t cloud_pin_doubles = 0;
    int cloud_pending = -1;
    bool cloud_direct_on = !(getenv("TDLO_DIRECT_CLOUD") && atoi(getenv("TDLO_DIRECT_CLOUD")) == 0);
    // cloud views (tdlo_set_cloud_view): a host view is packed into cloud_pin in its own precision and widened by k_cloud_import, which reads the pinned
    // block in place, as k_prologue reads Xhost (measured faster than a copy in front of the kernel at 5 000, 50 000 and 2 000 000 points,
    // profiles/cloud_view_ab.txt).  TDLO_VIEW_INPLACE=0: the block is copied to the device first (into the slot's Xs, which the next prune rewrites
    // anyway) -- the comparator.  view_route: tdlo_debug_route_count 17 / 18
    bool view_inplace = !(getenv("TDLO_VIEW_INPLACE") && atoi(getenv("TDLO_VIEW_INPLACE")) == 0);
    long long view_route[2] = {0, 0};
    long long voxel_view_calls = 0;       // tdlo_cloud_view_voxel_grid calls that reached the kernels (tdlo_debug_route_count 21)
    hipEvent_t ev_view = nullptr;          // recorded on a view's ready_stream; the context's stream waits for it
    // early exit, one frame per call: how many iterations go out before the host first looks at the registration's state.  1 unless the caller
    // knows better -- tracking_step passes what the same registration took in the previous frame (consecutive frames of a tracker take about
    // the same number; capped: a wrong guess costs a no-op iteration, ~4 us, per iteration too many).  Consumed by the next run_frames.
    int iter_hint = 0, iter_hint_next = 0;      // (_next: of the registration whose first M-step this one launches ahead, PairNext::spec)
    bool iter_hint_on = !(getenv("TDLO_ITER_HINT") && atoi(getenv("TDLO_ITER_HINT")) == 0);
    bool lle_next_on = !(getenv("TDLO_LLE_NEXT") && atoi(getenv("TDLO_LLE_NEXT")) == 0);        // 0: the host forms every LLE regulariser (comparator)
    bool spec_force_timeout = getenv("TDLO_SPEC_FORCE_TIMEOUT") && atoi(getenv("TDLO_SPEC_FORCE_TIMEOUT")) != 0;   // test hook, see run_frames
    bool spec_on = !(getenv("TDLO_SPEC_MSTEP") && atoi(getenv("TDLO_SPEC_MSTEP")) == 0);        // 0: the paired registration's first M-step is launched when its priors exist (comparator)
    bool pair_sums_on = !(getenv("TDLO_PAIR_SUMS") && atoi(getenv("TDLO_PAIR_SUMS")) == 0);     // 0: the paired registration still runs its own first E-step (comparator)
    // the E-step with two points per lane (k_estep2, tdlo_estep2.hip) for clouds and batches that fill the GPU.  TDLO_ESTEP2=0: never (comparator: k_estep
    // everywhere), 1: wherever it is eligible, whatever the size (tests); unset: by size.  TDLO_ESTEP2_ROWS=8|16: rows of its membership tile.
    int estep2_mode = getenv("TDLO_ESTEP2") ? atoi(getenv("TDLO_ESTEP2")) : -1;
    int estep2_rows = (getenv("TDLO_ESTEP2_ROWS") && atoi(getenv("TDLO_ESTEP2_ROWS")) == 16) ? 16 : 8;
    int estep2_blocks = getenv("TDLO_ESTEP2_BLOCKS") ? atoi(getenv("TDLO_ESTEP2_BLOCKS")) : 0;
    bool xch_self = getenv("TDLO_XCH_SELF") && atoi(getenv("TDLO_XCH_SELF")) != 0;      // a lone rank of the one-shot exchange exchanges with its own inbox (tdlo_set_xch_self)
    bool boost_off_once = false;          // run_frames' retry: an fp64-mode E-step refused a share under the sigma-following (finer) limits -- this call repeats with the coarse ones
    long long boost_retries = 0;          // how often that happened (tdlo_debug_route_count 10)
    bool test_boost_fail = getenv("TDLO_TEST_BOOST_FAIL") && atoi(getenv("TDLO_TEST_BOOST_FAIL")) != 0;   // test hook: every fp64-mode call's first attempt has its shares refused under the boosted limits (set_iter_consts)
    // fp64 E-step of chains beyond 64 nodes: batches whose node window is wide go lane = node (tdlo_estep_wide.h); TDLO_ESTEP_WIDE=0: thread = point throughout (comparator)
    int estep_wide_min = getenv("TDLO_ESTEP_WIDE") ? (atoi(getenv("TDLO_ESTEP_WIDE")) > 0 ? atoi(getenv("TDLO_ESTEP_WIDE")) : (1 << 30)) : kEstepWideMin;
    // One launch per iteration (tdlo_iter_fused.hip: k_iter_fused = M-step ; next E-step) for the registrations fused_iter_eligible names.  TDLO_FUSED_ITER=0: never
    // (the two-launch loop, the comparator); =1: also beyond the point count up to which it is the default; unset: by eligibility.
    int fused_iter_mode = getenv("TDLO_FUSED_ITER") ? (atoi(getenv("TDLO_FUSED_ITER")) != 0 ? 1 : 0) : -1;
    long long fused_calls = 0;            // registrations run that way (tdlo_debug_route_count 14)
    // ... with k_iter_fused_w0 where the chain's step slots all fit wave 0 (up to 61 nodes).  TDLO_FUSED_W0=0: k_iter_fused for every chain (the comparator)
    bool fused_w0_on = !(getenv("TDLO_FUSED_W0") && atoi(getenv("TDLO_FUSED_W0")) == 0);
    long long fused_w0_calls = 0;         // registrations of the one-launch loop whose iterations were k_iter_fused_w0, as launch_iter_fused reports them (tdlo_debug_route_count 24)
    long long estep2_frames = 0;          // registrations whose E-step was k_estep2 (tdlo_debug_route_count 9)
    bool timing = false;                  // tdlo_set_timing: record the four events behind tdlo_stats.loop_ms / total_ms (~15 us per call)
    EnqueuePool *pool = nullptr;          // made by the first batch that runs on several streams
    // split-mode scratch
    int split_active = 0;
    double *xch_dmin = nullptr;      // caller-owned device memory of the device-resident N-split exchange (tdlo_split_bind_exchange)
    double *xch_sums = nullptr;
    // tdlo_split_run: the whole split registration driven from C++ (RCCL called directly, or the one-shot exchange)
    double *split_buf = nullptr;     // RCCL form: [init 2 | dmin M | sums 4M+2], all-reduced in place on the context's stream
    size_t split_buf_doubles = 0;
    void *own_comm = nullptr;        // communicator made by tdlo_rccl_comm_init (destroyed with the context)
    unsigned long long *xch_own = nullptr;     // one-shot exchange: this rank's inbox (tdlo_xch_create)
    size_t xch_own_words = 0;
    int xch_rank = 0, xch_nranks = 0, xch_mcap = 0, xch_cap_ranks = 0;
    unsigned long long *xch_peer[kMaxXchRanks] = {};
    std::vector<void *> xch_opened;  // peer inboxes opened from IPC handles (closed with the context)
    unsigned xch_calls = 0;          // epoch of the flags: one per registration, in lockstep on all ranks
};

namespace {

// Development aid (TDLO_TRACK_PROFILE=1): host wall time between marks, accumulated per mark and printed when a tracker is destroyed -- where
// a tracking_step's host time goes (scripts/ubench/track_cpp.cpp).  Off: one predictable branch per mark.
struct HostProf {
    static constexpr int kN = 16;
    const char *name[kN] = {"set_cloud call", "guide nodes", "prepare_frame #1", "enqueue prologue #1", "enqueue iteration #1", "wait #1", "results #1",
                            "traverse + priors", "prepare_frame #2", "enqueue prologue #2", "enqueue iteration #2", "wait #2", "results #2", "between registrations", "", ""};
    double us[kN] = {};
    long n[kN] = {};
    bool on = getenv("TDLO_TRACK_PROFILE") && atoi(getenv("TDLO_TRACK_PROFILE")) != 0;
    int base = 0;                        // 0 inside the first registration of a tracking_step, 6 inside the second
    std::chrono::steady_clock::time_point t0;
    void start() { if (on) t0 = std::chrono::steady_clock::now(); }
    void mark(int id) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        us[id] += std::chrono::duration<double, std::micro>(t1 - t0).count(); ++n[id];
        t0 = t1;
    }
    void report() {
        if (!on) return;
        double tot = 0;
        for (int i = 0; i < kN; ++i) if (n[i]) tot += us[i] / (double)n[i];
        fprintf(stderr, "trackdlo_hip host profile (us per call of the phase; sum %.1f):\n", tot);
        for (int i = 0; i < kN; ++i) if (n[i]) fprintf(stderr, "  %-24s %8.2f  x %ld\n", name[i], us[i] / (double)n[i], n[i]);
    }
};
HostProf g_prof;

int fail(tdlo_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    // a refused launch or attribute leaves HIP's per-thread "last error" set; the launchers of the NEXT call read it after their own
    // (successful) launches and would report this call's failure a second time
    if (code == TDLO_E_HIP) (void)hipGetLastError();
    return code;
}

#define HIPCHK(c, call)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((c), TDLO_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));   \
    } while (0)

// Waits for the stream.  TDLO_SPIN_US=n polls hipStreamQuery for the first n microseconds before it blocks.  Measured on the production-size
// tracking_step (N = 5 000, M = 45; scripts/ubench/track_cpp.cpp, scripts/gpu_track.py): with the stream markers of tdlo_set_timing on, the
// blocking wait wakes up late and polling helps (0.189 -> 0.178 ms per frame); WITHOUT them -- the C API's default -- hipStreamSynchronize is the
// faster one (C++ caller 0.129 against 0.143 ms per frame: the runtime spins by itself, and hipStreamQuery is the more expensive call).  Default: off.
hipError_t wait_stream(hipStream_t s) {
    static const int spin_us = getenv("TDLO_SPIN_US") ? atoi(getenv("TDLO_SPIN_US")) : 0;
    if (spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t e = hipStreamQuery(s);
            if (e != hipErrorNotReady) return e;
            if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > spin_us) break;
        }
    }
    return hipStreamSynchronize(s);
}

// Before a buffer kernels may still be reading or polling is replaced: the first stream, and the second one while something launched ahead
// into the twin slot may still run there (an abandoned launch keeps polling the spec word / reading the staged cloud for up to 2 s: ADVICE r04)
hipError_t drain_for_realloc(tdlo_ctx *c) {
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return e;
    if (c->stream2[0]) return hipStreamSynchronize(c->stream2[0]);      // (cheap when idle; only the growth path comes here)
    return hipSuccess;
}

// The context's growing staging buffers follow one rule: a buffer is replaced only by a larger one; what may still read or poll the old one is
// drained first; a failing allocation leaves {nullptr, 0} behind, never a dangling pointer for tdlo_destroy.
enum class Staging {
    Pinned,            // pinned host memory, contents left as they come
    PinnedZeroed,      // ... cleared (flags and epochs that kernels compare with start at 0)
    DeviceZeroed       // device memory, cleared on the context's stream; only that stream is drained
};
static int grow_staging(tdlo_ctx *c, double *&buf, size_t &have, size_t doubles, Staging kind) {
    if (doubles <= have) return 0;
    const bool dev = kind == Staging::DeviceZeroed;
    HIPCHK(c, dev ? hipStreamSynchronize(c->stream) : drain_for_realloc(c));
    if (buf) { if (dev) hipFree(buf); else hipHostFree(buf); }
    buf = nullptr; have = 0;
    if (dev) {
        HIPCHK(c, hipMalloc((void **)&buf, doubles * sizeof(double)));
        HIPCHK(c, hipMemsetAsync(buf, 0, doubles * sizeof(double), c->stream));
    } else {
        HIPCHK(c, hipHostMalloc((void **)&buf, doubles * sizeof(double), hipHostMallocDefault));
        if (kind == Staging::PinnedZeroed) std::memset(buf, 0, doubles * sizeof(double));
    }
    have = doubles;
    return 0;
}
int ensure_pin(tdlo_ctx *c, size_t doubles) { return grow_staging(c, c->pin, c->pin_doubles, doubles, Staging::Pinned); }
int ensure_pin2(tdlo_ctx *c, size_t doubles) { return grow_staging(c, c->pin2, c->pin2_doubles, doubles, Staging::Pinned); }
// (its last word is the spec flag a kernel launched ahead compares with its epoch)
int ensure_late(tdlo_ctx *c, size_t doubles) { return grow_staging(c, c->late_buf, c->late_doubles, doubles, Staging::PinnedZeroed); }
// (kernels of an earlier call may still report their progress into the old one: hence the drain)
int ensure_mbox(tdlo_ctx *c, size_t doubles) { return grow_staging(c, c->mbox, c->mbox_doubles, doubles, Staging::PinnedZeroed); }
int ensure_cloud_pin(tdlo_ctx *c, size_t doubles) {
    if (doubles <= c->cloud_pin_doubles) return 0;
    return grow_staging(c, c->cloud_pin, c->cloud_pin_doubles, (doubles + 4095) & ~(size_t)4095, Staging::Pinned);
}
int ensure_xfer(tdlo_ctx *c, size_t doubles) { return grow_staging(c, c->xfer, c->xfer_doubles, doubles, Staging::DeviceZeroed); }

// Waits until the M-steps of registration `epoch` have reported `min_it` completed iterations, or that the registration is done (need_done:
// only that).  *word = the progress word seen.  Returns 0; 1 when the stream has drained without that report (the caller falls back on the
// read-back copy); a negative code for a HIP error on the stream.  The wait spins on pinned host memory -- the M-step's own store is the
// earliest moment the host can know -- and looks at the stream only every 0.5 ms, so that a faulting kernel cannot hang the caller.
int mbox_wait(tdlo_ctx *c, hipStream_t stream, unsigned epoch, int min_it, bool need_done, unsigned long long *word) {
    const unsigned long long *w = (const unsigned long long *)(c->mbox + c->mbox_doubles - 2);
    auto t_chk = std::chrono::steady_clock::now();
    for (unsigned spins = 1;; ++spins) {
        const unsigned long long v = __atomic_load_n(w, __ATOMIC_ACQUIRE);
        if ((unsigned)(v >> 32) == epoch) {
            const bool done = (v >> 31) & 1u;
            if (done || (!need_done && (int)(v & 0x7fffffffu) >= min_it)) { *word = v; return 0; }
        }
        if ((spins & 255u) == 0) {
            const auto now = std::chrono::steady_clock::now();
            if (std::chrono::duration<double, std::micro>(now - t_chk).count() > 500.0) {
                t_chk = now;
                const hipError_t e = hipStreamQuery(stream);
                if (e == hipSuccess) {          // drained: whatever was going to be reported has been (the kernel's stores precede its completion)
                    const unsigned long long v2 = __atomic_load_n(w, __ATOMIC_ACQUIRE);
                    if ((unsigned)(v2 >> 32) == epoch && (((v2 >> 31) & 1u) || (!need_done && (int)(v2 & 0x7fffffffu) >= min_it))) { *word = v2; return 0; }
                    return 1;
                }
                if (e != hipErrorNotReady) return fail(c, TDLO_E_HIP, std::string("stream: ") + hipGetErrorString(e));
            }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
}

int ensure_points(tdlo_ctx *c, Slot &s, int n) {
    if (n <= s.cap_points) return 0;
    HIPCHK(c, drain_for_realloc(c));
    if (s.Xraw) hipFree(s.Xraw);
    if (s.Xs) hipFree(s.Xs);
    if (s.bucket) hipFree(s.bucket);
    if (s.blksum) hipFree(s.blksum);
    s.Xraw = nullptr; s.Xs = nullptr; s.bucket = nullptr; s.blksum = nullptr;     // a failing hipMalloc below must not leave
    s.cap_points = 0; s.N0 = 0;                                                      // dangling pointers for tdlo_destroy
    const size_t cap = ((size_t)n + 1023) & ~(size_t)1023;
    const size_t nb = cap / kBlock + 1;
    HIPCHK(c, hipMalloc((void **)&s.Xraw, 3 * cap * sizeof(double)));
    HIPCHK(c, hipMalloc((void **)&s.Xs, 3 * cap * sizeof(double)));
    HIPCHK(c, hipMalloc((void **)&s.bucket, cap * sizeof(unsigned short)));
    HIPCHK(c, hipMalloc((void **)&s.blksum, (nb + 2) * sizeof(double)));      // (+ 2: FrameDev::keep)
    s.cap_points = (int)cap;
    s.sorted_valid = false;
    return 0;
}

int ensure_nodes(tdlo_ctx *c, Slot &s, int M) {
    if (M <= s.cap_nodes) return 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (s.nodeblk) hipFree(s.nodeblk);
    s.nodeblk = nullptr; s.cap_nodes = 0;
    const int cap = std::max(M, 16);
    NodeCarve nc(cap);
    HIPCHK(c, hipMalloc((void **)&s.nodeblk, nc.total * sizeof(double)));
    HIPCHK(c, hipMemsetAsync(s.nodeblk, 0, nc.total * sizeof(double), c->stream));
    if (!s.sync) {
        HIPCHK(c, hipMalloc((void **)&s.sync, 256 * sizeof(unsigned)));
        HIPCHK(c, hipMemsetAsync(s.sync, 0, 256 * sizeof(unsigned), c->stream));
    }
    s.nodeblk_doubles = nc.total;
    s.cap_nodes = cap;
    return 0;
}

int ensure_nodes2(tdlo_ctx *c, Slot &s, int M) {
    if (M <= s.cap_nodes2) return 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (s.nodeblk2) hipFree(s.nodeblk2);
    s.nodeblk2 = nullptr; s.cap_nodes2 = 0;
    const int cap = std::max(M, 16);
    NodeCarve nc(cap);
    HIPCHK(c, hipMalloc((void **)&s.nodeblk2, nc.total * sizeof(double)));
    HIPCHK(c, hipMemsetAsync(s.nodeblk2, 0, nc.total * sizeof(double), c->stream));
    s.cap_nodes2 = cap;
    return 0;
}

int ensure_hb_next(tdlo_ctx *c, Slot &s, int M) {
    if (M <= s.hb_next_cap) return 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (s.hb_next) hipFree(s.hb_next);
    s.hb_next = nullptr; s.hb_next_cap = 0; s.hb_next_valid = false;
    const int cap = std::max(M, 64);
    HIPCHK(c, hipMalloc((void **)&s.hb_next, sizeof(double) * 13 * (size_t)cap));
    s.hb_next_cap = cap;
    return 0;
}

// a cloud staged in pinned memory that no prologue has taken to the device goes there by a copy
int flush_pending_cloud(tdlo_ctx *c) {
    if (c->cloud_pending < 0) return 0;
    Slot &s = c->slots[c->cloud_pending];
    c->cloud_pending = -1;
    HIPCHK(c, hipMemcpyAsync(s.Xraw, c->cloud_pin, 3 * (size_t)s.N0 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return 0;
}

// the word a speculatively launched M-step waits on (FrameDev::spec_flag): the last double of the late-priors buffer
unsigned long long *spec_flag_word(tdlo_ctx *c) { return (unsigned long long *)(c->late_buf + c->late_doubles - 1); }
void spec_release(tdlo_ctx *c, unsigned epoch, bool go) {
    __atomic_store_n(spec_flag_word(c), ((unsigned long long)epoch << 32) | (go ? 1ull : 2ull), __ATOMIC_RELEASE);
}
// whatever happens to the call that launched it, a waiting M-step is told to leave
void spec_abort(tdlo_ctx *c) {
    if (c->pair.spec) { spec_release(c, c->pair.spec_epoch, false); c->pair.spec = 0; }
}

// the number the next fused prologue on this slot carries in its barrier word ((epoch << 1) | abandoned: 31 bits, never 0); bit 31 of the kernel
// argument is the test hook that withholds one arrival
unsigned next_fuse_epoch(tdlo_ctx *c, Slot &sl) {
    sl.fuse_epoch = sl.fuse_epoch >= 0x7fffffffu ? 1u : sl.fuse_epoch + 1u;
    if (c->fuse_force_timeout > 0 && --c->fuse_force_timeout == 0) return sl.fuse_epoch | 0x80000000u;
    return sl.fuse_epoch;
}

// A registration came back with TDLO_E_FUSE: its fused prologue's grid barrier was abandoned (not all workgroups of the launch became resident
// within 2 s).  Nothing of the caller's has been touched.  Everything in flight is told to leave and drained, what the abandoned launch left
// half-made is invalidated (the slots' sorted clouds, the barrier's arrival counter), and the context takes the copy + three-kernel route from now on.
void fuse_fallback(tdlo_ctx *c) {
    spec_abort(c);
    c->pair.state = 0; c->pair.ahead = false; c->pair.has_sums = false;
    (void)hipStreamSynchronize(c->stream);
    if (c->stream2[0]) (void)hipStreamSynchronize(c->stream2[0]);
    c->twin_busy = false;
    auto reset = [&](Slot &sl) {
        sl.sorted_valid = false;
        if (sl.sync) (void)hipMemsetAsync(sl.sync + 100, 0, 2 * sizeof(unsigned), c->stream);      // arrivals, barrier word (the epochs go on counting)
    };
    for (Slot &sl : c->slots) reset(sl);
    reset(c->twin);
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    if (c->fuse_on)
        std::fprintf(stderr, "trackdlo_hip: the fused prologue's workgroups were not co-resident within 2 s (device %d); this context now uses the "
                             "copy + three-kernel route (see INTEGRATION.md, co-residency)\n", c->device);
    c->fuse_on = false;
    ++c->route_count[5];
}

bool same_params(const tdlo_params &a, const tdlo_params &b) {
    return a.beta == b.beta && a.lambda == b.lambda && a.lle_weight == b.lle_weight && a.mu == b.mu && a.max_iter == b.max_iter && a.tol == b.tol &&
           a.include_lle == b.include_lle && a.alpha == b.alpha && a.k_vis == b.k_vis && a.visibility_threshold == b.visibility_threshold &&
           a.precision == b.precision;
}

int check_params(tdlo_ctx *c, int M, const tdlo_params *p) {
    if (!p) return fail(c, TDLO_E_INVALID, "params is null");
    if (M < 4) return fail(c, TDLO_E_INVALID, "M < 4: the reference's neighbour clamps (trackdlo.cpp:313-321) need at least 4 nodes");
    if (M > kMaxNodes) return fail(c, TDLO_E_INVALID, "M > 1024 is not supported by the E-step tiling");
    if (p->max_iter < 0) return fail(c, TDLO_E_INVALID, "max_iter < 0");
    if (p->precision != TDLO_PREC_F32 && p->precision != TDLO_PREC_F64) return fail(c, TDLO_E_INVALID, "bad precision");
    // the kernel G of trackdlo.cpp:233 divides by beta; a negative lambda makes the M-step's system indefinite (the reference's launch files use
    // 0.35 / 3.0 and 50 000 / 1).  lambda == 0 is legal there (A = D G, least-squares solve): it takes the dense eliminations (prepare_frame).
    if (!(p->beta > 0.0)) return fail(c, TDLO_E_INVALID, "beta must be positive (kernel G of trackdlo.cpp:233)");
    if (!(p->lambda >= 0.0)) return fail(c, TDLO_E_INVALID, "lambda must not be negative");
    return 0;
}

// J / Y_extended (trackdlo.cpp:240-260) into a frame's staging block: aJ = alpha * diag(J), aYd = alpha * (Y_extended - Y0)
int stage_priors(tdlo_ctx *c, double *aJ, double *aYd, const double *Y, int M, const double *priors, int K, double alpha) {
    std::fill(aJ, aJ + M, 0.0);
    std::fill(aYd, aYd + 3 * M, 0.0);
    for (int i = 0; i < K; ++i) {
        const int idx = (int)priors[4 * i];
        if (idx < 0 || idx >= M) return fail(c, TDLO_E_INVALID, "correspondence prior index out of range");
        aJ[idx] = alpha;
        for (int d = 0; d < 3; ++d) aYd[d * M + idx] = alpha * (priors[4 * i + 1 + d] - Y[d * M + idx]);
    }
    return 0;
}

// Fills the host-side upload block [Yin | aJ | aYd | H] for one frame and its FrameDev.
// k_estep2 (two points per lane) can serve this frame: fp32 mode, chains of 8 .. 64 nodes
// How many replica rows of the accumulators a frame's E-step workgroups spread their atomics over (FrameDev::acc_rows).  More rows: fewer atomics per address;
// fewer rows: less for the one-workgroup M-step to fetch in the round trip every iteration waits for.  Measured on one box (scripts/gpu_ab.sh; the rows first as
// a build constant 2 / 4 / 8, then -- with the M-step told its iteration's parity, which halves the fetch on its own -- through TDLO_ACC_ROWS):
//   C5 (782 workgroups of an fp64 E-step of 14 us, uneven work; 1 202 sums): M-step 17.59 / 17.73 / 18.14 us, E-step the same -> 2;
//   C2 (196 workgroups, fp32): E-step 5.26 / 4.60 / 4.52 us as a constant; with the parity known, iteration 13.13 (4 rows) against 12.99 us (8) -> 8;
//   C4 (977 workgroups of equal work, finishing together): E-step 17.7 (4) against 16.95 us (8) -> 8.
// The totals are integers: every choice gives the same bits.  Only the plain one-frame chain M-step is instantiated for fewer rows (tdlo_mstep_chain.hip);
// every other M-step adds up all eight (the unused ones are zero).  TDLO_ACC_ROWS=2|4|8 overrides.
static void choose_acc_rows(const tdlo_ctx *c, FrameDev &f, bool merged) {
    static const int env = getenv("TDLO_ACC_ROWS") ? atoi(getenv("TDLO_ACC_ROWS")) : 0;
    (void)c;
    int r = kAccRows;
    if (!merged && !f.include_lle && !f.mstep_dense && f.M > kChunk && f.M <= kChainLdsMaxNodes && f.precision == TDLO_PREC_F64) r = 2;
    if (env == 2 || env == 4 || env == 8) r = env;
    f.acc_rows = r;
}

// The loop with one launch per iteration (tdlo_iter_fused.hip): ONE frame in fp32 mode on the chain M-step (no LLE term, TDLO_MSTEP not dense), 8 .. 64 nodes, no
// visibility term (k_dmin would sit between the two halves), k_estep with the one-frame tile (not k_estep2), results through the mailbox, none of tracking_step's
// short cuts -- and a cloud whose E-step has fewer waves than the GPU has SIMDs (65 536 points): there the E-step is a chain of latencies, and every workgroup
// repeating the M-step costs no time; beyond, the E-step's workgroups take several batches each and the M-step in front of each is issue time (TDLO_FUSED_ITER=1
// takes those too).  What run_frames adds: not a batch, not a paired / ahead / late-priors registration.
constexpr int kFusedIterMaxPoints = 65536;
static bool fused_iter_eligible(const tdlo_ctx *c, const FrameDev &f) {
    return c->fused_iter_mode != 0 && f.precision == TDLO_PREC_F32 && !f.include_lle && !f.mstep_dense && f.M >= 8 && f.M <= kChunk && !f.vis_branch &&
           f.estep2 == 0 && f.wide_tile != 0 && f.eb == 256 && f.max_iter > 0 && f.host_prog != nullptr && f.lle_next == nullptr && f.spec_flag == nullptr &&
           f.late_aJ == nullptr && f.pair_sums == nullptr && f.xch_nranks == 0 && (c->fused_iter_mode == 1 || f.N0 <= kFusedIterMaxPoints);
}

static bool estep2_eligible(const tdlo_ctx *c, const FrameDev &f) {
    return c->estep2_mode != 0 && f.precision == TDLO_PREC_F32 && f.M >= 8 && f.M <= kChunk;
}
// ... and does: the launch geometry of a frame whose E-step is k_estep2.  `share`: the frame is one of a batch (the batch fills the GPU, every
// wave takes two 128-point batches so that a workgroup's prologue and epilogue are paid half as often -- as k_estep's batches do).
static void estep2_geometry(tdlo_ctx *c, FrameDev &f, bool share) {
    if (!f.estep2) {
        ++c->estep2_frames;
        // the fixed point's grain is one wave x one 128-point batch here: a node's P1 share can reach 128 (prepare_frame sized the exponents for
        // 64), and Q is converted per PAIR of points -- one binary digit less keeps every conversion exact (|v 2^sh| < 2^51); the totals' bound
        // (2^62) only gains from it
        for (int k = 0; k < 3; ++k) { f.acc_sh[k] -= 1; f.acc_lim[k] *= 2.0; }
    }
    f.estep2 = c->estep2_rows;
    f.wide_tile = 0; f.eb = 256;
    const int nb128 = (f.N0 + 127) / 128;
    int nblk = (nb128 + 3) / 4;
    if (share && nblk >= 32) nblk = (nblk + 1) / 2;
    // One frame: every workgroup resident at once (five of 28 KB and 86 VGPRs per CU: 1280 on 256 CUs) and every wave the SAME number of batches -- first
    // the batches per wave that fits the cloud into the resident waves, then the workgroups that many batches need.  (N = 2 000 000: 15 625 batches, 4 per
    // wave, 977 workgroups.  1280 workgroups gave waves of 3 and of 4 batches -- 19.0 us per E-step against 16.9 with 1024 or 1536, scripts/gpu_estep2_sweep.sh.)
    const int cap = c->estep2_blocks > 0 ? c->estep2_blocks : (c->cfg.estep_blocks > 0 ? c->cfg.estep_blocks : 1280);
    if (nblk > cap) { const int per_wave = (nb128 + 4 * cap - 1) / (4 * cap); nblk = (nb128 + 4 * per_wave - 1) / (4 * per_wave); }
    f.nblkE = std::max(1, std::min(nblk, std::min(cap, kMaxEstepBlocks)));
}

// trackdlo.cpp:358: visible_nodes.size() != Y.rows() && !visible_nodes.empty() && k_vis != 0 -- the registration weighs the memberships by visibility
static bool frame_vis_branch(int n_vis, int M, const tdlo_params *p) { return n_vis != M && n_vis != 0 && p->k_vis != 0; }

int prepare_frame(tdlo_ctx *c, int slot, const double *Y, int M, double sigma2, const tdlo_params *p,
                  const double *priors, int K, const int *vis, int n_vis, const double *H_override,
                  double *stage, FrameDev &f, bool second_block = false, bool hb_may_stay = true) {      // hb_may_stay: f.Hb may point at Slot::hb_next (a batch moves every frame's Hb into its transfer buffer instead)
    Slot &s = slot < 0 ? c->twin : c->slots[slot];      // (slot < 0: the context's twin slot, PairNext::ahead)
    if (s.N0 <= 0) return fail(c, TDLO_E_INVALID, "no cloud resident in slot (call tdlo_set_cloud)");
    int rc = second_block ? ensure_nodes2(c, s, M) : ensure_nodes(c, s, M);
    if (rc) return rc;
    NodeCarve nc(M);
    double *blk = second_block ? s.nodeblk2 : s.nodeblk;
    std::memcpy(stage + nc.Yin, Y, sizeof(double) * 3 * M);
    {
        const int prc = stage_priors(c, stage + nc.aJ, stage + nc.aYd, Y, M, priors, K, p->alpha);
        if (prc) return prc;
    }
    bool lle_band = false, h_banded = false, hb_resident = false;
    double band_s2_max = 1e300;
    if (p->include_lle) {
        double *H = stage + nc.H;
        // The banded L D L^T in the chain's state (tdlo_mstep_band.hip) serves the registration when (i) H is banded like the
        // reference's own (I - L)^T (I - L) -- +-6 nodes; an H_override may be anything --, (ii) it is symmetric there (the band is read
        // from one triangle), (iii) no two consecutive nodes are closer than h_min: the state precision K contains Q^-1 ~ 3 beta^4 / h^3, and
        // the solve's error grows like eps lambda sigma2 K / P1: at h = 1 mm with the pre-processing parameters (beta 3, lambda 1)
        // 1e-13 m, at 0.1 mm 1e-11 m, at 0.01 mm 1e-7 m (scripts/band_gap_study.py); the bound scales with cbrt(lambda beta^4).
        // Everything else (coincident nodes in particular: K is infinite there) keeps the dense pivoted eliminations.
        if (mstep_band_enabled() && !c->lle_dense_once && !c->lle_batch_dense && p->lambda > 0 && p->beta > 0 && M <= kChainLdsMaxNodes) {      // (the banded solve keeps a record per unknown in LDS: up to 512 nodes)
            lle_band = true;
            const double hmin = 1e-3 * std::cbrt(p->lambda * std::pow(p->beta / 3.0, 4));
            double hsum = 0;
            for (int i = 0; i + 1 < M && lle_band; ++i) {
                double d2 = 0;
                for (int d = 0; d < 3; ++d) { const double e = Y[d * M + i + 1] - Y[d * M + i]; d2 += e * e; }
                if (!(d2 >= hmin * hmin)) lle_band = false;
                hsum += std::sqrt(d2);
            }
            // (iv) fp64 mode only: K's entries ~ 3 beta^4 / h^3 are rounded to fp64 when the records are formed, and a smooth displacement field
            // cancels in K x to many digits -- the rounding comes back divided by the data term, ~ eps sigma2 K |x| / P1.  At the reference's scale
            // (sigma2 <= 1e-2 m2) that is 1e-13 m; a registration started from sigma2 = 0 on a chain of 8 .. 10 m begins at sigma2 = 3 .. 6 m2 and
            // with beta = 5 the banded form -- ANY fp64 solve of the stored band: scripts/gpu_band_cond_study.py, DESIGN.md 4 -- is 1.4 .. 5.5e-9 m
            // from the reference's dense system, outside the mode's 1e-9 m.  Measured onset sigma2 beta^4 ~ 1 500 at h = 2 cm; the bound sits a
            // factor 3 below and scales with K.  A sigma2 given by the caller is checked here, one computed on the device (sigma2 == 0,
            // trackdlo.cpp:271-273) by the M-step itself (FrameDev::band_s2_max), which ends in the repeat on the dense kernels (run_frames).
            band_s2_max = 1e300;
            if (lle_band && p->precision == 1 && M > 1) {
                const double hm = hsum / (M - 1);
                band_s2_max = 6.25e7 * hm * hm * hm / std::pow(p->beta, 4);
                if (sigma2 > band_s2_max) lle_band = false;
            }
            if (H_override) {
                for (int j = 0; j < M && lle_band; ++j)
                    for (int i = 0; i < M; ++i) {
                        const double v = H_override[(size_t)j * M + i];
                        if ((std::abs(i - j) > 6 && v != 0.0) || v != H_override[(size_t)i * M + j] || !(v == v)) { lle_band = false; break; }
                    }
            }
        }
        if (lle_band) {
            // the banded solve reads H through its 13 diagonals only (Hb[13 i + u] = H(i, i - 6 + u)): the M x M matrix is neither formed nor uploaded
            double *Hb = stage + nc.Hb;
            if (H_override) {
                for (int i = 0; i < M; ++i)
                    for (int u = 0; u < 13; ++u) { const int j = i - 6 + u; Hb[(size_t)13 * i + u] = (j >= 0 && j < M) ? H_override[(size_t)j * M + i] : 0.0; }
            } else if (c->lle_next_on && hb_may_stay && !second_block && s.hb_next_valid && s.hb_next_Y.size() == 3 * (size_t)M &&
                       std::memcmp(s.hb_next_Y.data(), Y, sizeof(double) * 3 * M) == 0) {
                hb_resident = true;                          // formed on the device at the end of the previous tracking_step (FrameDev::lle_next): the same values
            } else {
                lle_regulariser_band(Y, M, Hb);              // trackdlo.cpp:236-237, O(M)
            }
        } else if (H_override) {
            std::memcpy(H, H_override, sizeof(double) * (size_t)M * M);
            h_banded = true;
            for (int j = 0; j < M && h_banded; ++j)
                for (int i = 0; i < M; ++i) if (std::abs(i - j) > 6 && H_override[(size_t)j * M + i] != 0.0) { h_banded = false; break; }
        } else {
            h_banded = true;
            std::vector<double> L((size_t)M * M);
            lle_weights(6, Y, M, L.data());                  // trackdlo.cpp:236
            lle_regulariser(L.data(), M, H);                 // :237
        }
    }

    std::memset(&f, 0, sizeof f);
    f.N0 = s.N0; f.M = M; f.ldx = s.cap_points;
    const int nbatch = (s.N0 + 63) / 64;
    // 4 waves per workgroup (fp64 tiles are twice as large anyway; fp32: a cloud that cannot fill the GPU gets twice the workgroups of the
    // 8-wave form, one wave per SIMD -- C2: 5.6 -> 5.2 us per E-step -- and at N = 2 000 000 1024 workgroups of 4 waves beat 512 of 8 by
    // 4 %).  The results do not depend on this choice: the sums are integers from the grain of one wave x one batch on.
    f.eb = 256;
    { static const int eb_env = getenv("TDLO_ESTEP_EB") ? atoi(getenv("TDLO_ESTEP_EB")) : 0; if (eb_env == 256 || (eb_env == 512 && M <= 64 && p->precision == TDLO_PREC_F32)) f.eb = eb_env; }
    const int wpb = f.eb / 64;
    int nblk = (nbatch + wpb - 1) / wpb;
    // One frame of moderate size (up to 262 144 points) keeps its whole node window in a 64-row tile (67 KB of LDS per 4-wave
    // workgroup).  A larger cloud is VALU-bound instead: it takes the 24-row tile of the batch path (more workgroups per CU hide the
    // LDS / scalar-load latencies: 47 -> 36 us at N = 2 000 000).  Batches (run_frames, F > 1) always use the small tile.
    f.wide_tile = (M > kChunk || nbatch < 4096) ? 1 : 0;
    // (fp32, chains up to 64 nodes, a cloud that fills the GPU: 2048 workgroups of the 16-row tile -- 26.5 against 27.9 us per E-step at N = 2 000 000)
    int cap = c->cfg.estep_blocks > 0 ? c->cfg.estep_blocks : (f.wide_tile ? 512 : ((M <= kChunk && p->precision == TDLO_PREC_F32) ? 2048 : 1024));
    // (more than 64 nodes: the 24-row tile lets two fp64 workgroups share a CU -- C5: 512 workgroups 21.4 us per converged E-step and 69.7 us per
    //  iteration over a whole call, against 28.4 / 86.3 with 256 workgroups of the former 64-row tile, which filled a CU's LDS alone)
    { static const int cap_env = getenv("TDLO_ESTEP_BLOCKS") ? atoi(getenv("TDLO_ESTEP_BLOCKS")) : 0; if (cap_env > 0) cap = cap_env; }
    cap = std::min(cap, kMaxEstepBlocks);
    f.nblkE = std::max(1, std::min(nblk, cap));
    f.max_iter = p->max_iter; f.include_lle = p->include_lle ? 1 : 0; f.has_priors = K > 0 ? 1 : 0;
    // trackdlo.cpp:358: visible_nodes.size() != Y.rows() && !visible_nodes.empty() && k_vis != 0
    f.vis_branch = frame_vis_branch(n_vis, M, p) ? 1 : 0;
    (void)vis;
    f.precision = p->precision;
    // which M-step: decided here, once per frame (the launchers dispatch on the descriptor, not on the process-wide toggles)
    f.mstep_dense = (mstep_chain_enabled() && p->lambda > 0.0) ? 0 : 1;      // (the chain smoother works in units of 1 / (lambda sigma2))
    f.lle_band = lle_band ? 1 : 0;
    f.band_s2_max = band_s2_max;
    f.h_banded = h_banded ? 1 : 0;
    f.need_G = ((p->include_lle && !lle_band) || (!p->include_lle && f.mstep_dense)) ? 1 : 0;
    {   // test hook: iteration k of the multi-CU M-steps behaves as if a hand-off had timed out (tests/test_parity_gpu.py)
        static const int force_it = getenv("TDLO_MCU_FORCE_TIMEOUT") ? atoi(getenv("TDLO_MCU_FORCE_TIMEOUT")) : -1;
        f.force_timeout_it = force_it;
    }
    // prune / counting-sort workgroups: 256 points each up to 1024 workgroups; larger clouds give every workgroup 2, 4, 8 ...
    // consecutive tiles, so that the one-workgroup scan of the (workgroup, node) histogram in k_setup stays ~1000 rows
    f.prune_tiles = 1;
    while ((s.N0 + kBlock * f.prune_tiles - 1) / (kBlock * f.prune_tiles) > 1024) f.prune_tiles *= 2;
    f.nprune_blocks = (s.N0 + kBlock * f.prune_tiles - 1) / (kBlock * f.prune_tiles);
    {   // the E-step's node window in bits (FrameDev::win_e32): TDLO_WINDOW=exact keeps every membership that is not exactly zero in the arithmetic
        static const bool exact = getenv("TDLO_WINDOW") && getenv("TDLO_WINDOW")[0] == 'e';
        f.win_e32 = exact ? 154.0 : 36.0; f.win_e64 = exact ? 1100.0 : 66.0;
    }
    f.tol = p->tol; f.beta = p->beta; f.lambda = p->lambda; f.lle_weight = p->lle_weight; f.mu = p->mu;
    f.alpha = p->alpha; f.k_vis = p->k_vis; f.vis_thr = p->visibility_threshold; f.sigma2_in = sigma2;
    {   // per (prune block, node) histogram of the counting sort
        const size_t need = (size_t)f.nprune_blocks * M;
        if (need > s.hist_ints) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (s.hist) hipFree(s.hist);
            s.hist = nullptr; s.hist_ints = 0;
            HIPCHK(c, hipMalloc((void **)&s.hist, 2 * need * sizeof(int)));       // counts | start offsets
            s.hist_ints = need;
        }
    }
    f.Xraw = s.Xraw; f.Xs = s.Xs; f.bucket = s.bucket; f.hist = s.hist; f.hist_off = s.hist + (size_t)f.nprune_blocks * M; f.blksum = s.blksum;
    f.keep = s.blksum + (size_t)s.cap_points / kBlock + 1;
    f.reuse_sorted = (c->sort_reuse && s.sorted_valid && s.sorted_prec == p->precision && s.sorted_Y.size() == 3 * (size_t)M &&
                      std::memcmp(s.sorted_Y.data(), Y, sizeof(double) * 3 * M) == 0) ? 1 : 0;
    f.Yin = blk + nc.Yin; f.ctr = blk + nc.ctr; f.Y = blk + nc.Y; f.Y0 = blk + nc.Y0; f.nodes = blk + nc.nodes;
    f.coord = blk + nc.coord; f.G = blk + nc.G; f.chain = blk + nc.chain; f.H = blk + nc.H; f.Hb = blk + nc.Hb; f.HG = blk + nc.HG; f.HY0 = blk + nc.HY0;
    f.aJ = blk + nc.aJ; f.aYd = blk + nc.aYd; f.dminbits = (unsigned long long *)(blk + nc.dmin);
    f.acc = (long long *)(blk + nc.acc);
    f.band = blk + nc.band;
    {   // fixed-point exponents of the accumulators: totals stay below 2^62.  P1_m <= N0.  |R_m| <= sum_n P_mn |x_n - y_m| <= N0 D and
        // Q <= N0 D^2 with D a bound on point-node distances: every kept point is within 0.1 m of a node (:177-195), nodes are within
        // the chain's length of each other; doubled for the motion of the nodes during the registration, rounded up to a power of two
        int ln = 0; while (((long long)1 << ln) < (long long)s.N0 + 1) ++ln;
        double len = 0;
        for (int i = 0; i + 1 < M; ++i) { double d2 = 0; for (int d = 0; d < 3; ++d) { const double e = Y[d * M + i + 1] - Y[d * M + i]; d2 += e * e; } len += std::sqrt(d2); }
        int ld = 0; while (std::ldexp(1.0, ld) < 2.0 * (len + 0.2) && ld < 20) ++ld;
        // ... and one wave's share of one 64-point batch below 2^51 (acc_fix): P1 <= 64, |R| <= 64 D, a point's share of Q <= D^2
        static const int sh_coarser = getenv("TDLO_ACC_COARSER") ? atoi(getenv("TDLO_ACC_COARSER")) : 0;      // experiment: how much of a deviation from the oracle is the sums' resolution (scripts/gpu_acc.py)
        const int shP = std::min(60 - ln, 44) - sh_coarser;
        f.acc_sh[0] = shP; f.acc_sh[1] = shP - ld; f.acc_sh[2] = shP - 2 * ld;
        {   // (experiment, with TDLO_ACC_COARSER: only one class of sums coarser)
            static const int only = getenv("TDLO_ACC_COARSER_ONLY") ? atoi(getenv("TDLO_ACC_COARSER_ONLY")) : -1;
            if (only >= 0) for (int k = 0; k < 3; ++k) if (k != only) f.acc_sh[k] += sh_coarser;
        }
        // D is a heuristic (nodes can be pulled anywhere by a prior, a diverging registration leaves it): the E-step CHECKS every value it
        // converts against these limits -- the conversion stays exact below 2^51, the sum of all batches' shares (P1, R: one per 64-point
        // batch and node; Q: one per point) below 2^62 -- and ends the registration with TDLO_E_NUMERIC beyond them, as it does for NaN
        const int lshare = std::min(51, 67 - std::max(ln, 6)), lpoint = std::min(51, 61 - ln);
        f.acc_lim[0] = std::ldexp(1.0, lshare - f.acc_sh[0]); f.acc_lim[1] = std::ldexp(1.0, lshare - f.acc_sh[1]); f.acc_lim[2] = std::ldexp(1.0, lpoint - f.acc_sh[2]);
    }
    f.acc_boost_off = c->boost_off_once ? 1 : (c->test_boost_fail ? -1 : 0);      // (-1: the test hook of set_iter_consts)
    f.estep_wide_min = c->estep_wide_min;
    // (acc_rows: choose_acc_rows, once the E-step's geometry is final)
    // one frame whose cloud fills the GPU alone (2048 waves of 64 points: from there on two points per lane win, scripts/gpu_estep2_check.py /
    // profiles/r06_measured.log -- 131 072 points 4.8 against 5.3 us per E-step, 250 000 points (a shard of C4 on eight ranks) 5.5 against 7.3 us)
    if (estep2_eligible(c, f) && (c->estep2_mode == 1 || nbatch >= kEstep2MinWaves)) estep2_geometry(c, f, false);
    choose_acc_rows(c, f, false);
    f.sums = blk + nc.sums; f.Ascr = blk + nc.Ascr; f.Yout = blk + nc.Yout; f.dbg = (unsigned long long *)(blk + nc.dbg);
    f.sync = s.sync;
    f.st = (IterState *)(blk + nc.st);
    if (hb_resident) f.Hb = s.hb_next;
    return 0;
}

// the E-step's fixed-point accumulators of these frames, both parities (the measurement entry points restart the iteration counter)
hipError_t zero_accumulators(const std::vector<FrameDev> &fh, int F, hipStream_t s) {
    for (int i = 0; i < F; ++i) {
        const hipError_t e = hipMemsetAsync(fh[i].acc, 0, sizeof(long long) * 2 * kAccRows * (4 * (size_t)fh[i].M + 2), s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

size_t upload_doubles(const NodeCarve &nc, const tdlo_params *p, bool band) { return p->include_lle ? (band ? nc.H : nc.upload) : nc.Hb; }

void fill_stats(tdlo_stats *st, const IterState &is) {
    st->iters = is.it; st->converged = is.converged; st->n_kept = is.N; st->status = is.status; st->sigma2 = is.sigma2;
    st->mstep_retries = is.retries;
}

// Priors formed by the host while the set-up kernel of the registration runs (tracking_step's second registration: they come out of the first
// registration's result through traverse_euclidean, 6.5 us of host time that used to sit between the two registrations).  Returns 0 and the
// K x 4 rows, or an error code.
typedef std::function<int(const double *&, int &)> LatePriors;

// the mailbox epoch of the next registration that reports there (never 0: a cleared mailbox carries 0)
static unsigned next_mbox_epoch(tdlo_ctx *c) {
    unsigned e = ++c->mbox_epoch;
    if (e == 0) e = ++c->mbox_epoch;
    return e;
}

// The descriptor of a main registration's first M-step that is launched AHEAD of its priors (FrameDev::spec_flag), from the registration's own
// descriptor PairNext::f: the priors will come through the late buffer, the results go to the mailbox under `epoch`.  spec_prev: the state of the
// pre-processing registration whose end it waits for (nullptr: the host's word alone); lle_next: where the M-step that finishes the registration
// leaves the next frame's LLE regulariser (nullptr: nowhere).
static FrameDev spec_mstep_descriptor(tdlo_ctx *c, const tdlo_ctx::PairNext &pn, unsigned epoch, const IterState *spec_prev, double *lle_next) {
    FrameDev fs = pn.f;
    fs.reuse_sorted = 1; fs.has_priors = 1;
    fs.late_aJ = c->late_buf; fs.late_aYd = c->late_buf + pn.M;
    fs.host_out = c->mbox; fs.host_prog = (unsigned long long *)(c->mbox + c->mbox_doubles - 2); fs.host_epoch = epoch;
    fs.host_report_it = (pn.p.tol <= 0.0 || pn.p.max_iter <= 2 * kChunkIters) ? 0 : std::max(1, std::min(std::min(c->iter_hint_next, kIterHintMax), pn.p.max_iter));
    fs.spec_flag = spec_flag_word(c); fs.spec_prev = spec_prev; fs.spec_epoch = epoch;
    if (lle_next) fs.lle_next = lle_next;
    return fs;
}

// PairNext::ahead (tracking_step with hidden nodes; called by the pre-processing registration's run_frames once its own first iterations are on the
// first stream): the main registration's fused prologue, k_dmin and first E-step on the SECOND stream, in the context's twin slot -- they read
// the frame's cloud from the pinned staging buffer like the pre-processing registration's own prologue -- and its first M-step behind them, waiting
// for the priors.  Returns 0 whether or not it launched anything (PairNext::state == 2 && ahead says it did); a negative code for a HIP error.
static int launch_ahead(tdlo_ctx *c) {
    tdlo_ctx::PairNext &pn = c->pair;
    const int M = pn.M;
    const int N0 = c->slots[pn.slot].N0;
    const NodeCarve nc(M);
    if (!pn.cloud_in_pin || N0 <= 0 || pn.p.include_lle || pn.p.max_iter <= 0 || M > kChainLdsMaxNodes) return 0;
    if (c->late_doubles < 4 * (size_t)M + 2 || c->mbox_doubles < nc.readback + 4 || c->cloud_pin_doubles < 3 * (size_t)N0) return 0;      // (sized by tracking_step before anything was launched)
    if (!c->stream2[0]) HIPCHK(c, hipStreamCreateWithFlags(&c->stream2[0], hipStreamNonBlocking));
    hipStream_t sb = c->stream2[0];
    Slot &tw = c->twin;
    const size_t need_hist = (size_t)((N0 + kBlock - 1) / kBlock) * M;
    const bool grow = N0 > tw.cap_points || M > tw.cap_nodes || need_hist > tw.hist_ints || nc.upload + 2 > c->pin2_doubles;
    if (grow || c->twin_busy) HIPCHK(c, hipStreamSynchronize(sb));      // (buffers about to be replaced, or a staging block an abandoned launch may still be reading)
    c->twin_busy = false;
    int rc;
    if ((rc = ensure_points(c, tw, N0))) return rc;
    tw.N0 = N0; tw.sorted_valid = false;
    if ((rc = ensure_pin2(c, nc.upload + 2))) return rc;
    FrameDev &f = pn.f;
    if ((rc = prepare_frame(c, -1, pn.Y.data(), M, pn.sigma2, &pn.p, nullptr, 0, nullptr, pn.n_vis, nullptr, c->pin2, f, false))) return rc;
    if (grow) HIPCHK(c, hipStreamSynchronize(c->stream));               // (new buffers are cleared on the first stream)
    if (!f.wide_tile || f.mstep_dense || f.reuse_sorted || !c->fuse_on || !prologue_pair_ok(f)) return 0;      // not this frame: the main registration takes the ordinary route
    pn.up = upload_doubles(nc, &pn.p, false);
    f.Xhost = c->cloud_pin;
    std::memcpy(c->pin2 + nc.fdev, &f, sizeof(FrameDev));
    const unsigned fep = next_fuse_epoch(c, tw);
    c->twin_busy = true;
    HIPCHK(c, launch_prologue_direct(&f, c->pin2, tw.nodeblk, (int)pn.up, (int)nc.Yin, fep, sb));
    f.Xhost = nullptr;                      // (the cloud is in the twin's Xraw for everything that follows)
    f.late_mstep = 1;                       // the priors do not exist yet: this E-step leaves them alone, the M-step reads them itself
    const FrameDev *fdb = (const FrameDev *)(tw.nodeblk + nc.fdev);
    if (f.vis_branch) HIPCHK(c, launch_estep_only(fdb, &f, 1, 1, sb));
    HIPCHK(c, launch_estep_only(fdb, &f, 1, 0, sb));
    const unsigned e2 = next_mbox_epoch(c);
    const FrameDev fs = spec_mstep_descriptor(c, pn, e2, nullptr, nullptr);
    HIPCHK(c, launch_mstep_chain(fdb, &fs, 1, 0, fs.precision == TDLO_PREC_F64, sb));
    pn.has_sums = false; pn.spec = 1; pn.spec_epoch = e2; pn.ahead = true; pn.state = 2;
    return 0;
}

// iterations of early-exit chunk number `chunk`: 1, 1, 2, 4, 4, ... and no more than are left
static int chunk_iters(int chunk, int left) { return std::min(chunk < 2 ? 1 : (chunk == 2 ? 2 : kChunkIters), left); }

// frame i's state in an array of read-back blocks [Yout | IterState] in host memory, `stride` doubles apart
static IterState readback_state(const double *blocks, size_t stride, const NodeCarve &nc, int i) {
    IterState is;
    std::memcpy(&is, blocks + (size_t)i * stride + (nc.st - nc.Yout), sizeof is);
    return is;
}
static bool every_frame_done(const double *blocks, size_t stride, const NodeCarve &nc, int F) {
    for (int i = 0; i < F; ++i) if (readback_state(blocks, stride, nc, i).done == 0) return false;
    return true;
}
static bool any_frame_ended_with(int status, const double *blocks, size_t stride, const NodeCarve &nc, int F) {
    for (int i = 0; i < F; ++i) if (readback_state(blocks, stride, nc, i).status == status) return true;
    return false;
}

int run_frames(tdlo_ctx *c, int F, const int *slots, double *Y, int M, double *sigma2, const tdlo_params *p,
               const double *priors, int K, const int *vis, int n_vis, const double *H_override, tdlo_stats *stats,
               const LatePriors *late = nullptr, const tdlo_frame_args *each = nullptr);

// a paired registration's first M-step may already be waiting on the stream (launched by the previous call): released when the priors are staged,
// told to leave on every other way out of run_frames
struct SpecGuard {
    tdlo_ctx *c; unsigned epoch = 0; bool live = false;
    void release(bool go) { if (live) { spec_release(c, epoch, go); live = false; } }
    ~SpecGuard() { release(false); }
};

// One call of run_frames: its arguments, what it has decided and how far it has come.  The member functions are run_frames' phases, in the order
// run_frames calls them; each returns 0 or the call's error code.
struct FramesCall {
    // the arguments
    tdlo_ctx *const c; const int F; const int *const slots; double *const Y; const int M; double *const sigma2; const tdlo_params *const p;
    // priors / visible set / H per frame (F entries): the caller's own (tdlo_cpd_lle_batch_each, a batch of trackers), or the call's shared ones F times
    std::vector<tdlo_frame_args> fa;
    tdlo_stats *const stats;
    const LatePriors *const late;
    const int iter_hint;          // tdlo_ctx::iter_hint as this call found it
    const bool timing;
    // layout.  Batches move their host-supplied blocks and their results with ONE copy each way: every small copy is a 4-5 us blit kernel on the
    // stream, and 32 frames x (upload + read-back [+ flags per polling chunk]) had grown to 0.3 ms of a 2.3 ms call.  The frames' [Yin | aJ | aYd | H]
    // and [Yout | IterState] then live in one device buffer instead of the slots' node blocks (the kernels only see pointers).
    const NodeCarve nc;
    const bool merged;
    // how much of a frame's block travels: without the LLE term up to Hb; with it the 13 diagonals Hb when the banded solve serves the call, else
    // the dense H as well.  A batch is staged at the stride of the banded form first; a frame the banded solve cannot take sends the whole
    // batch to the dense kernels (one M-step kernel per launch), and the frames are staged again at the full stride.
    size_t up, ustride;
    // the frame descriptors ride in the same host-to-device copy: one frame -> at the head of its upload block, a batch -> as an array
    // behind the F upload blocks (every separate small copy is a blit kernel plus a dependent-dispatch gap, ~4 us)
    const size_t fdd;             // doubles of the descriptor array of a batch
    // route
    bool paired = false;          // tracking_step's second registration whose node-side set-up the first one's prologue has already done (PairNext)
    bool ahead = false;           // ... or whose whole first iteration up to the M-step has run beside the previous registration, in the twin slot (PairNext::ahead)
    bool use_mbox = false;        // the results come back through the pinned mailbox
    bool fused_mode = false;      // one launch per iteration (tdlo_iter_fused.hip)
    bool fused_w0_seen = false;   // ... and one of them was k_iter_fused_w0: the registration is counted once (tdlo_debug_route_count 24)
    bool late_async = false;      // the late priors are formed beside the set-up kernel
    bool lle_next = false;        // the M-step that finishes the registration leaves the next frame's LLE regulariser behind
    // streams
    hipStream_t s = nullptr;      // the call's first stream
    hipStream_t gs[kBatchStreams] = {};
    int goff[kBatchStreams + 1] = {};
    int NS = 1;
    bool forked = false;
    // progress
    int enqueued = 0;             // iterations this call has put on the stream (or released)
    bool sums_first = false;      // the first iteration is its M-step alone, from the sums the previous registration's first M-step left
    bool ahead_first = false;     // the first iteration is on the second stream already: its M-step waits for the priors staged by this call
    bool spec_released = false;   // ... and that M-step had been launched ahead and was released by this call
    unsigned epoch = 0;           // of the mailbox
    bool have_readback = false;   // the results are already in pinned memory (early exit after the first iteration; the mailbox)
    const FrameDev *fdp = nullptr;      // this call's descriptors on the device
    double *nodeblk_used = nullptr;     // one frame: the node block the registration runs out of
    SpecGuard sg;

    FramesCall(tdlo_ctx *c_, int F_, const int *slots_, double *Y_, int M_, double *sigma2_, const tdlo_params *p_, const double *priors_, int K_,
               const int *vis_, int n_vis_, const double *H_override_, tdlo_stats *stats_, const LatePriors *late_, int iter_hint_,
               const tdlo_frame_args *each_)
        : c(c_), F(F_), slots(slots_), Y(Y_), M(M_), sigma2(sigma2_), p(p_),
          fa(each_ ? std::vector<tdlo_frame_args>(each_, each_ + (F_ > 0 ? F_ : 0)) : std::vector<tdlo_frame_args>(F_ > 0 ? F_ : 0, tdlo_frame_args{priors_, K_, vis_, n_vis_, H_override_})),
          stats(stats_), late(late_), iter_hint(iter_hint_), timing(c_->timing), nc(M_), merged(F_ > 1),
          up(upload_doubles(nc, p_, p_->include_lle && mstep_band_enabled() && !c_->lle_dense_once)), ustride(merged ? up : nc.upload),
          fdd(((size_t)F_ * sizeof(FrameDev) + 15) / 16 * 2), sg{c_} {}

    Slot &slot0() const { return c->slots[slots[0]]; }
    size_t rstride() const { return merged ? nc.readback : nc.upload; }      // of the read-back blocks in tdlo_ctx::pin
    bool fixed_count() const { return p->tol <= 0.0 || p->max_iter <= 2 * kChunkIters; }

    int size_staging();
    void recognise_pair();
    int stage_frames();
    int choose_batch_kernels();
    int choose_routes();
    int open_mailbox();
    int upload_and_prologue();
    int stage_late_priors();
    int fork_streams();
    void choose_loop();
    int drive_fixed();
    int drive_mailbox();
    int drive_polled();
    int read_back();
    bool repeat(int *rc);
    int results_out(std::chrono::steady_clock::time_point t_host0);

    FrameDev fused_copy(int k) const;
    hipError_t iterate(int n);
    hipError_t join();
    int mbox_done(int min_it, bool need_done, bool *done);
    int take_mbox(bool events_recorded);
    int launch_paired_mstep_ahead();
};

int FramesCall::size_staging() {
    int rc = ensure_pin(c, (size_t)F * std::max(nc.upload, nc.readback + 2) + fdd + 2 * (size_t)F * std::max(nc.readback, (sizeof(IterState) + 7) / 8) + 4);
    if (rc) return rc;
    if (merged) rc = ensure_xfer(c, (size_t)F * (upload_doubles(nc, p, false) + nc.readback) + fdd);
    return rc;
}

// tracking_step's second registration whose node-side set-up the first one's prologue has already done (PairNext): same slot, nodes, sigma2 and
// parameters as were set up, on the cloud that was sorted for these nodes -- then nothing is staged and no prologue is launched
void FramesCall::recognise_pair() {
    if (late && c->pair.state == 2) {
        const tdlo_ctx::PairNext &pn = c->pair;
        const Slot &sl = slot0();
        const bool same = F == 1 && !fa[0].priors && !fa[0].H_override && pn.slot == slots[0] && pn.M == M && pn.n_vis == fa[0].n_vis && pn.sigma2 == sigma2[0] && same_params(pn.p, *p) &&
                          std::memcmp(pn.Y.data(), Y, sizeof(double) * 3 * M) == 0 && pn.f.wide_tile != 0;
        if (pn.ahead) paired = ahead = same && c->stream2[0] != nullptr;
        else paired = same && sl.sorted_valid && sl.sorted_prec == p->precision &&
                      sl.sorted_Y.size() == 3 * (size_t)M && std::memcmp(sl.sorted_Y.data(), Y, sizeof(double) * 3 * M) == 0;
        c->pair.state = 0; c->pair.ahead = false;
    }
    if (late && c->pair.spec) { sg.epoch = c->pair.spec_epoch; sg.live = true; c->pair.spec = 0; }
    if (!paired) sg.release(false);
    c->fh.assign(F, FrameDev{});
    if (paired) {
        c->fh[0] = c->pair.f; c->fh[0].reuse_sorted = 1; up = c->pair.up;
        if (ahead) ++c->route_count[4];
        else { ++c->route_count[0]; if (c->pair.has_sums) ++c->route_count[1]; }
    }
}

// every frame's upload block and descriptor, in up to two passes: banded LLE form first, the dense one if a frame of the batch cannot take it
int FramesCall::stage_frames() {
    for (int pass = 0; pass < 2 && !paired; ++pass) {
        for (int i = 0; i < F; ++i) {
            const tdlo_frame_args &a = fa[i];
            const int rc = prepare_frame(c, slots[i], Y + (size_t)i * 3 * M, M, sigma2[i], p, a.priors, a.K, a.visible_nodes, a.n_vis, a.H_override,
                                         c->pin + (size_t)i * ustride, c->fh[i], false, !merged);
            if (rc) return rc;
            if (merged) {
                FrameDev &f = c->fh[i];
                f.wide_tile = 0;
                // batches fill the GPU: half the workgroups per frame, every wave takes two 64-point batches -- the per-workgroup prologue (nodes
                // to LDS) and epilogue (wave sums, atomics) are paid half as often (32 frames: 879 k -> 991 k it/s in the loop).  The sums do
                // not depend on how batches are dealt out (integer accumulation): with k_estep on both sides the results are those of the single
                // call, bit for bit.  A batch that fills the GPU takes k_estep2 below (128-point grain, one binary digit less) where the frame
                // alone takes k_estep: then each frame's sums are the single call's within the E-step's own rounding, not bit for bit.
                if (c->cfg.estep_blocks <= 0 && f.nblkE >= 64) f.nblkE = (f.nblkE + 1) / 2;
                double *bu = c->xfer + (size_t)i * up, *br = c->xfer + (size_t)F * up + fdd + (size_t)i * nc.readback;
                f.Yin = bu + nc.Yin; f.aJ = bu + nc.aJ; f.aYd = bu + nc.aYd;
                if (p->include_lle) { f.Hb = bu + nc.Hb; f.H = bu + nc.H; }
                f.Yout = br; f.st = (IterState *)(br + (nc.st - nc.Yout));
            }
        }
        if (merged) { const int rc = choose_batch_kernels(); if (rc) return rc; }
        if (!p->include_lle) break;
        bool all_band = true;
        for (int i = 0; i < F; ++i) all_band = all_band && c->fh[i].lle_band;
        if (all_band) break;
        if (!merged) { up = upload_doubles(nc, p, false); break; }      // one frame: its block was staged at the full stride anyway
        if (pass == 0) { c->lle_batch_dense = true; up = upload_doubles(nc, p, false); ustride = up; }
    }
    c->lle_batch_dense = false;
    return 0;
}

// what a batch decides once for all its frames: the E-step kernel and the replica rows of the accumulators
int FramesCall::choose_batch_kernels() {
    // a batch whose frames together fill the GPU takes the E-step with two points per lane (one choice for the whole launch)
    long long waves = 0;
    bool elig = true;
    for (int i = 0; i < F; ++i) { waves += (c->fh[i].N0 + 63) / 64; elig = elig && estep2_eligible(c, c->fh[i]); }
    const bool two = elig && (c->estep2_mode == 1 || waves >= kEstep2MinWaves);
    for (int i = 0; i < F; ++i) if (two) estep2_geometry(c, c->fh[i], true);      // (a frame prepare_frame had given to k_estep2 on its own size keeps it only if the whole batch does:
    for (int i = 0; i < F; ++i) choose_acc_rows(c, c->fh[i], true);
    // a batch of short fp32 chains without the LLE term whose frames have at most 64 E-step workgroups each (C3: 49): two replica rows -- no more atomics
    // per address than one 50 000-point frame puts on eight -- and a quarter of the sums for every frame's M-step to fetch (one choice for the whole batch)
    {
        static const int env = getenv("TDLO_ACC_ROWS") ? atoi(getenv("TDLO_ACC_ROWS")) : 0;
        bool small = env == 0 && !p->include_lle;
        for (int i = 0; i < F; ++i) small = small && c->fh[i].nblkE <= 64 && !c->fh[i].mstep_dense && c->fh[i].M <= kChunk;
        if (small) for (int i = 0; i < F; ++i) c->fh[i].acc_rows = 2;
    }
    // the E-step and k_dmin are instantiated per launch with or without the visibility weights (trackdlo.cpp:358): frames with per-frame visible sets that
    // disagree here are split into two calls by the entry points (run_frames_each)
    for (int i = 1; i < F; ++i) if (c->fh[i].vis_branch != c->fh[0].vis_branch) return fail(c, TDLO_E_INVALID, "internal: a batch's frames disagree about the visibility weights");
    if (!two) for (int i = 0; i < F; ++i) if (c->fh[i].estep2) return fail(c, TDLO_E_INVALID, "internal: a batch's frames disagree about the E-step kernel");   //  same M, precision and mode -- they cannot)
    return 0;
}

// what tracking_step's short cuts add to the descriptor, the late priors that cannot ride beside the set-up kernel, the sort reused per launch
int FramesCall::choose_routes() {
    if (!merged && !paired && p->include_lle && c->fh[0].lle_band && slot0().hb_next != nullptr && c->fh[0].Hb == slot0().hb_next)
        { up = nc.Hb; ++c->route_count[3]; }      // H's 13 diagonals are on the device already (Slot::hb_next): they do not travel
    // tracking_step's main registration: the M-step that finishes it leaves the next frame's LLE regulariser behind (FrameDev::lle_next; the
    // buffer was sized by tracking_step before anything was launched)
    lle_next = late != nullptr && !merged && !ahead && c->lle_next_on && !p->include_lle && !c->fh[0].mstep_dense && M <= 256 && p->max_iter > 0 &&
               slot0().hb_next_cap >= M;      // (ahead: its first M-step is on the second stream already, without this job -- and the next frame's
                                              //  pre-processing registration, on the first stream, must not race it)
    if (lle_next) { c->fh[0].lle_next = slot0().hb_next; slot0().hb_next_valid = false; }
    // Late priors ride beside the set-up kernel only where the E-step can hand them to the M-step (the one-frame kernel, which takes the frame
    // descriptor by value): otherwise they are formed here, before anything is launched, and staged like ordinary ones.
    late_async = late != nullptr && c->fh[0].wide_tile != 0 && (c->late_on || paired);
    if (late && !late_async) {
        const double *lp = nullptr; int lk = 0;
        int rc;
        if ((rc = (*late)(lp, lk))) return rc;
        if ((rc = stage_priors(c, c->pin + nc.aJ, c->pin + nc.aYd, Y, M, lp, lk, p->alpha))) return rc;
        c->fh[0].has_priors = lk > 0 ? 1 : 0;
    }
    g_prof.mark(g_prof.base + 2);
    {   // prune, scan and scatter are skipped per LAUNCH: the sorted clouds are reused only when every frame of the call can reuse its own
        // (a frame that skipped its scan while the batch's scatter ran would have its cloud re-scattered from stale start offsets)
        bool all_reuse = true;
        for (int i = 0; i < F; ++i) all_reuse = all_reuse && c->fh[i].reuse_sorted;
        if (!all_reuse) for (int i = 0; i < F; ++i) c->fh[i].reuse_sorted = 0;
    }
    return 0;
}

// One frame per call on a one-workgroup M-step (the chain smoother, the banded LLE solve): the results come back through the pinned
// mailbox -- the M-step that finishes the registration writes them there itself -- instead of a copy and a stream synchronisation
int FramesCall::open_mailbox() {
    use_mbox = !merged && c->mbox_on && p->max_iter > 0 &&
               ((!p->include_lle && !c->fh[0].mstep_dense) || (p->include_lle && c->fh[0].lle_band));
    if (!use_mbox) { sg.release(false); return 0; }
    const int rc = ensure_mbox(c, nc.readback + 4);
    if (rc) return rc;
    epoch = sg.live ? sg.epoch : next_mbox_epoch(c);         // (the waiting M-step reports under the epoch it was launched with)
    c->fh[0].host_out = c->mbox; c->fh[0].host_prog = (unsigned long long *)(c->mbox + c->mbox_doubles - 2); c->fh[0].host_epoch = epoch;
    return 0;
}

// the host-supplied blocks to the device and the prologue (prune, sort, set-up) behind them, on one of three routes: set up by the previous
// call (paired), one launch that reads the block from pinned host memory, or a copy and the three kernels
int FramesCall::upload_and_prologue() {
    int rc;
    s = ahead ? c->stream2[0] : c->stream;      // (a registration that began on the second stream stays there: its kernels are ordered by the stream)
    if (timing) HIPCHK(c, hipEventRecord(c->ev[0], s));
    if (merged) {
        std::memcpy(c->pin + (size_t)F * up, c->fh.data(), sizeof(FrameDev) * F);
        HIPCHK(c, hipMemcpyAsync(c->xfer, c->pin, ((size_t)F * up + fdd) * sizeof(double), hipMemcpyHostToDevice, s));
        fdp = (const FrameDev *)(c->xfer + (size_t)F * up);
    } else {
        if (!paired) std::memcpy(c->pin + nc.fdev, c->fh.data(), sizeof(FrameDev));
        nodeblk_used = ahead ? c->twin.nodeblk : (paired ? slot0().nodeblk2 : slot0().nodeblk);
        fdp = (const FrameDev *)(nodeblk_used + nc.fdev);
    }
    if (c->cloud_pending >= 0) {
        // tracking_step staged this frame's cloud in pinned host memory: the fused prologue reads it from there; any other route gets a copy first
        const bool fused = !merged && !paired && c->direct_in && c->fuse_on && c->cloud_pending == slots[0] && !c->fh[0].reuse_sorted && prologue_pair_ok(c->fh[0]);
        if (fused) { c->fh[0].Xhost = c->cloud_pin; c->cloud_pending = -1; }
        else if ((rc = flush_pending_cloud(c))) return rc;
    }
    if (paired) {
        // (set up by the previous call's prologue)
    } else if (!merged && c->direct_in && (c->fuse_on || c->fh[0].reuse_sorted) && prologue_direct_ok(c->fh[0])) {
        // one small frame (or a reused sort): ONE launch reads the block from pinned host memory, puts it in its place and does the whole prologue
        Slot &sl = slot0();
        const unsigned fep = c->fh[0].reuse_sorted ? 0u : next_fuse_epoch(c, sl);      // (a reused sort: the set-up workgroup alone, no barrier)
        // tracking_step asked for the set-up of its second registration to ride along (PairNext): staged like a frame of its own into the second
        // pinned block / the slot's second node block, one more workgroup of the fused prologue
        tdlo_ctx::PairNext &pn = c->pair;
        const FrameDev *f2 = nullptr;
        if (pn.state == 1) {
            pn.state = 0;
            if (!late && !c->fh[0].reuse_sorted && prologue_pair_ok(c->fh[0]) && pn.slot == slots[0] && pn.M == M && !pn.p.include_lle) {
                const NodeCarve nc2(pn.M);
                if ((rc = ensure_pin2(c, nc2.upload + 2))) return rc;
                if ((rc = prepare_frame(c, pn.slot, pn.Y.data(), pn.M, pn.sigma2, &pn.p, nullptr, 0, nullptr, pn.n_vis, nullptr, c->pin2, pn.f, true))) return rc;
                if (pn.f.wide_tile && !pn.f.mstep_dense && !pn.f.vis_branch) {
                    pn.up = upload_doubles(nc2, &pn.p, false);
                    std::memcpy(c->pin2 + nc2.fdev, &pn.f, sizeof(FrameDev));
                    f2 = &pn.f;
                    // the two registrations' first E-steps are the same computation (see FrameDev::pair_sums) when they share nodes, sigma2, mu and
                    // precision and neither weighs by visibility; the banded M-step of THIS registration then hands the sums over
                    pn.has_sums = p->include_lle && c->fh[0].lle_band && !c->fh[0].vis_branch && p->mu == pn.p.mu && p->precision == pn.p.precision &&
                                  sigma2[0] == pn.sigma2 && std::memcmp(Y, pn.Y.data(), sizeof(double) * 3 * M) == 0 && p->max_iter > 0 && c->pair_sums_on;
                    if (pn.has_sums) c->fh[0].pair_sums = sl.nodeblk2 + nc2.sums;
                }
            }
        }
        HIPCHK(c, launch_prologue_direct(c->fh.data(), c->pin, sl.nodeblk, (int)up, (int)nc.Yin, fep, s, f2, c->pin2, sl.nodeblk2, f2 ? (int)pn.up : 0));
        c->fh[0].Xhost = nullptr;          // (the cloud is in Xraw for everything that follows)
        if (f2) pn.state = 2;
    } else {
        if (!merged) HIPCHK(c, hipMemcpyAsync(slot0().nodeblk, c->pin, up * sizeof(double), hipMemcpyHostToDevice, s));
        bool scan = false;
        if (c->prologue_scan_on) HIPCHK(c, launch_prologue_scan(fdp, c->fh.data(), F, s, &scan));
        if (scan) ++c->prologue_scan_calls;
        else HIPCHK(c, launch_prune_and_setup(fdp, c->fh.data(), F, s));
    }
    g_prof.mark(g_prof.base + 3);
    for (int i = 0; i < F; ++i) {           // the slots' sorted clouds now belong to these nodes (recorded as soon as the prologue is enqueued: whatever fails later, the device's sort is this one)
        Slot &sl = c->slots[slots[i]];
        if (!c->fh[i].reuse_sorted) { sl.sorted_Y.assign(Y + (size_t)i * 3 * M, Y + (size_t)(i + 1) * 3 * M); sl.sorted_prec = p->precision; sl.sorted_valid = true; }
    }
    return 0;
}

// the set-up kernel is on its way (it copies the staging block as it is: the priors' part is overwritten by the E-step's copy of what
// follows); now the host forms the priors and puts them where the first E-step fetches them
int FramesCall::stage_late_priors() {
    if (late_async) {
        const double *lp = nullptr; int lk = 0;
        int rc = (*late)(lp, lk);
        if (!rc) rc = ensure_late(c, 4 * (size_t)M);
        if (!rc) rc = stage_priors(c, c->late_buf, c->late_buf + M, Y, M, lp, lk, p->alpha);
        if (rc) { sg.release(false); (void)hipStreamSynchronize(s); return rc; }        // (the set-up kernel reads the pinned staging block: drained before anybody reuses it)
        if (lk <= 0) sg.release(false);                    // (it was launched expecting priors)
        c->fh[0].has_priors = lk > 0 ? 1 : 0;
        c->fh[0].late_aJ = c->late_buf; c->fh[0].late_aYd = c->late_buf + M;
        g_prof.mark(7);
    }
    if (timing) HIPCHK(c, hipEventRecord(c->ev[1], s));
    return 0;
}

// A batch runs as up to kBatchStreams groups of frames on as many streams, each group one E-step behind the previous
// one: a batch's M-step is one workgroup per frame (F of the 256 CUs busy for 17 us), and meanwhile the other groups'
// E-steps have the rest of the GPU.  The groups are independent registrations: the results do not depend on the split
// (TDLO_BATCH_STREAMS=1 disables it).
int FramesCall::fork_streams() {
    static const int ns_env = getenv("TDLO_BATCH_STREAMS") ? atoi(getenv("TDLO_BATCH_STREAMS")) : 0;
    // (32 frames: three groups of 11 / 11 / 10 frames -- 1078 workgroups per E-step launch, about what the GPU holds at once -- give 1.155 M it/s against
    // 1.129 M for four groups of 8, three runs each, on one box and 1.124 M against 1.118 M on another; 24 frames: four groups 0.93 M against 0.91 M; 48 frames: three groups 1.26 M against 1.18 M)
    NS = ns_env > 0 ? ns_env : (F >= 28 ? 3 : (F >= 16 ? 4 : (F >= 8 ? 2 : 1)));
    NS = std::max(1, std::min(std::min(NS, kBatchStreams), F));
    for (int g = 0; g <= NS; ++g) goff[g] = (int)(((long long)F * g) / NS);
    gs[0] = s;
    for (int g = 1; g < NS; ++g) {            // the further streams are made when a batch first needs them: a context that only ever
        if (!c->stream2[g - 1]) HIPCHK(c, hipStreamCreateWithFlags(&c->stream2[g - 1], hipStreamNonBlocking));   // registers single frames
        gs[g] = c->stream2[g - 1];            // (or a shard) occupies one hardware queue, not four
    }
    return 0;
}

// how the first iteration starts, and whether the loop is the one with one launch per iteration (tdlo_iter_fused.hip): iteration k of the call is
// `M-step (k) ; E-step (k + 1)` in one kernel, behind a plain k_estep for iteration 0; the registration's last M-step is a k_mstep_chain on its own.
// Launch k reads copy k & 1 of state / Y / Yout / nodes and writes the other one.
void FramesCall::choose_loop() {
    sums_first = paired && !ahead && c->pair.has_sums;
    ahead_first = ahead;
    fused_mode = !merged && F == 1 && !paired && !ahead && late == nullptr && c->pair.state == 0 && use_mbox && !sums_first && !ahead_first &&
                 fused_iter_eligible(c, c->fh[0]);
    if (fused_mode) ++c->fused_calls;
}

FrameDev FramesCall::fused_copy(int k) const {
    FrameDev fc = c->fh[0];           // (as it stands now: host_report_it changes from chunk to chunk)
    if (k & 1) { double *blk = nodeblk_used; fc.Yout = blk + nc.Yout2; fc.st = (IterState *)(blk + nc.st2); fc.Y = blk + nc.Y2; fc.nodes = blk + nc.nodes2; }
    return fc;
}

// the next n iterations onto the stream(s)
hipError_t FramesCall::iterate(int n) {
    for (int it = 0; it < n; ++it) {
        ++enqueued;
        if (fused_mode) {
            const int k = enqueued - 1;
            if (k == 0) TDLO_RET(launch_estep_only(fdp, c->fh.data(), 1, 0, s));
            if (k + 1 < p->max_iter) {
                bool ran_w0 = false;
                TDLO_RET(launch_iter_fused(fused_copy(k), fused_copy(k + 1), k, c->fused_w0_on, s, &ran_w0));
                if (ran_w0 && !fused_w0_seen) { fused_w0_seen = true; ++c->fused_w0_calls; }      // (what the launcher launched, not what the host expects of it)
            }
            else TDLO_RET(launch_mstep_chain_close(fused_copy(k), k, s));
            continue;
        }
        if (sums_first || ahead_first) {
            const bool from_given = sums_first;
            sums_first = false; ahead_first = false;
            // test hook (tdlo_ctx::spec_force_timeout): the M-step launched ahead is told to leave instead of being released, as if it had given up waiting (2 s without the host)
            if (sg.live) { sg.release(!c->spec_force_timeout); spec_released = true; if (!ahead) ++c->route_count[2]; }      // it is on the stream already: the priors are staged, off it goes
            else if (from_given) TDLO_RET(launch_mstep_chain(fdp, c->fh.data(), 1, 1, c->fh[0].precision == TDLO_PREC_F64, s));
            else {          // (ahead, and the waiting M-step was sent away -- no priors after all --: it has cleared its E-step's sums, an ordinary iteration follows it)
                c->fh[0].late_mstep = 0;
                TDLO_RET(launch_iteration(fdp, c->fh.data(), 1, s));
            }
            c->fh[0].late_mstep = 0;               // (later M-steps find the priors in the node block, where the first one put them)
            continue;
        }
        for (int g = 0; g < NS; ++g) {
            const FrameDev *fdg = fdp + goff[g], *fhg = c->fh.data() + goff[g];
            const int Fg = goff[g + 1] - goff[g];
            if (NS > 1 && !forked && g + 1 < NS) {
                // first iteration, kernel by kernel (same kernels, same order as launch_iteration), so that the next group
                // can be released when this group's first E-step has drained
                if (fhg[0].vis_branch) TDLO_RET(launch_estep_only(fdg, fhg, Fg, 1, gs[g]));
                TDLO_RET(launch_estep_only(fdg, fhg, Fg, 0, gs[g]));
                TDLO_RET(hipEventRecord(c->evx[g], gs[g]));
                TDLO_RET(hipStreamWaitEvent(gs[g + 1], c->evx[g], 0));
                TDLO_RET(launch_estep_only(fdg, fhg, Fg, 2, gs[g]));
            } else {
                TDLO_RET(launch_iteration(fdg, fhg, Fg, gs[g], enqueued - 1));      // (this call's count of the registration's iterations: mstep_parity_hint)
            }
        }
        forked = true;
    }
    return hipSuccess;
}

// everything enqueued on the other streams so far precedes what follows on the first
hipError_t FramesCall::join() {
    if (NS < 2 || !forked) return hipSuccess;
    for (int g = 1; g < NS; ++g) {
        TDLO_RET(hipEventRecord(c->evj[g - 1], gs[g]));
        TDLO_RET(hipStreamWaitEvent(s, c->evj[g - 1], 0));
    }
    return hipSuccess;
}

// waits for the mailbox to report min_it iterations (need_done: the end of the registration); *done: the registration has ended
int FramesCall::mbox_done(int min_it, bool need_done, bool *done) {
    unsigned long long w = 0;
    int wr = mbox_wait(c, s, epoch, min_it, need_done, &w);
    if (wr == 1 && spec_released) {
        // The M-step launched ahead of its priors gave up waiting for them (this thread was held up for more than the kernel's 2 s) and left
        // without touching anything; what was enqueued behind it ran as a registration that does its own first E-step.  The state on the
        // device says where that stands: the iterations this call believes to be on the stream are made up, the ordinary way.
        spec_released = false;
        IterState is;
        HIPCHK(c, hipMemcpy(&is, c->fh[0].st, sizeof is, hipMemcpyDeviceToHost));
        int have = is.it;
        // (ahead: the M-step that left has cleared its E-step's sums -- ordinary iterations from the start)
        if (!ahead && !is.done && have == 0 && enqueued > 0) { HIPCHK(c, launch_mstep_chain(fdp, c->fh.data(), 1, 1, c->fh[0].precision == TDLO_PREC_F64, s)); have = 1; }
        for (; !is.done && have < enqueued; ++have) HIPCHK(c, launch_iteration(fdp, c->fh.data(), 1, s));
        wr = mbox_wait(c, s, epoch, min_it, need_done, &w);
    }
    if (wr < 0) return wr;
    if (wr == 1) return fail(c, TDLO_E_HIP, "the stream drained, but the M-step did not report the state of the registration");
    *done = (w >> 31) & 1u;
    return 0;
}

// the mailbox's read-back block into the staging buffer, where the results are read from
int FramesCall::take_mbox(bool events_recorded) {
    std::memcpy(c->pin, c->mbox, nc.readback * sizeof(double));
    have_readback = true;
    if (timing) {
        if (!events_recorded) { HIPCHK(c, hipEventRecord(c->ev[2], s)); HIPCHK(c, hipEventRecord(c->ev[3], s)); }
        HIPCHK(c, hipEventSynchronize(c->ev[3]));
    }
    return 0;
}

// fixed iteration count: enqueue everything, no host involvement.  Several stream groups and enough iterations: the first
// iteration (which releases the groups one after the other) from this thread, the rest of every group from a thread of its own.
int FramesCall::drive_fixed() {
    static const bool pool_on = !(getenv("TDLO_BATCH_THREADS") && atoi(getenv("TDLO_BATCH_THREADS")) == 0);
    int rc;
    if (NS > 1 && pool_on && p->max_iter >= 8) {
        HIPCHK(c, iterate(1));
        if (!c->pool) { c->pool = new EnqueuePool; c->pool->start(kBatchStreams - 1, c->device); }
        const int rest = p->max_iter - 1;
        const int prc = c->pool->run([&](int g) -> int {
            if (g >= NS) return 0;
            const FrameDev *fdg = fdp + goff[g], *fhg = c->fh.data() + goff[g];
            const int Fg = goff[g + 1] - goff[g];
            for (int it = 0; it < rest; ++it) { const hipError_t e = launch_iteration(fdg, fhg, Fg, gs[g], 1 + it); if (e != hipSuccess) return (int)e; }
            return 0;
        });
        if (prc) return fail(c, TDLO_E_HIP, std::string("batch enqueue: ") + hipGetErrorString((hipError_t)prc));
    } else {
        HIPCHK(c, iterate(p->max_iter));
    }
    if (use_mbox) {
        if (timing) { HIPCHK(c, hipEventRecord(c->ev[2], s)); HIPCHK(c, hipEventRecord(c->ev[3], s)); }      // behind the last iteration, as the read-back path does
        bool done = false;
        if ((rc = mbox_done(0, true, &done))) return rc;
        if ((rc = take_mbox(true))) return rc;
    }
    return 0;
}

// tracking_step's main registration starts with its M-step (PairNext::has_sums): launched NOW, behind the pre-processing registration's first
// iteration -- a steady-state tracker converges in it -- and ahead of the priors it needs (FrameDev::spec_flag)
int FramesCall::launch_paired_mstep_ahead() {
    tdlo_ctx::PairNext &pn = c->pair;
    Slot &sl = slot0();
    const NodeCarve nc2(pn.M);
    const int rc = ensure_late(c, 4 * (size_t)pn.M + 2);         // (may drain the stream: before anything waits on it)
    if (rc) return rc;
    const unsigned e2 = next_mbox_epoch(c);
    const bool leaves_lle = c->lle_next_on && pn.M <= 256 && sl.hb_next_cap >= pn.M;      // (as the registration itself will set it, choose_routes)
    const FrameDev fs = spec_mstep_descriptor(c, pn, e2, c->fh[0].st, leaves_lle ? sl.hb_next : nullptr);
    HIPCHK(c, launch_mstep_chain((const FrameDev *)(sl.nodeblk2 + nc2.fdev), &fs, 1, 1, fs.precision == TDLO_PREC_F64, s));
    pn.spec = 1; pn.spec_epoch = e2;
    return 0;
}

// early exit (trackdlo.cpp:424-428), decided on the device and read from the mailbox: the first iteration is checked eagerly (a tracker
// in steady state converges in it) -- or the first `iter_hint` iterations, when the caller knows how many the registration took last time
// (tdlo_ctx::iter_hint) --; after that iterations go out in chunks of 1, 1, 2, 4, 4, ... and the host looks at the progress
// word of the chunk BEFORE the one it has just enqueued, so that the GPU never idles (kernels of a finished registration are no-ops)
int FramesCall::drive_mailbox() {
    int rc;
    const int first = std::max(1, std::min(std::min(iter_hint, kIterHintMax), p->max_iter));
    c->fh[0].host_report_it = first;       // (the frame descriptor travels by value with every launch of the one-frame kernels)
    HIPCHK(c, iterate(first));
    if (!late && c->pair.state == 2 && c->pair.has_sums && c->spec_on && c->mbox_on && !timing && c->pair.p.max_iter > 0) {
        if ((rc = launch_paired_mstep_ahead())) return rc;
    } else if (!late && c->pair.state == 3) {
        // tracking_step with hidden nodes: the main registration's first iteration goes out NOW, on the second stream, beside this registration
        c->pair.state = 0; c->pair.ahead = false;
        if (c->spec_on && c->mbox_on && !timing && c->pair.slot == slots[0] && (rc = launch_ahead(c))) { spec_abort(c); return rc; }
    }
    g_prof.mark(g_prof.base + 4);
    bool stop = false;
    if ((rc = mbox_done(first, false, &stop))) { spec_abort(c); return rc; }
    if (!stop && !c->pair.ahead) c->pair.spec = 0;           // (this registration goes on: the waiting M-step has seen that and left; one launched AHEAD keeps waiting)
    g_prof.mark(g_prof.base + 5);
    int launched = first;
    for (int chunk = 0; launched < p->max_iter && !stop; ++chunk) {
        const int n = chunk_iters(chunk, p->max_iter - launched);
        c->fh[0].host_report_it = launched + n;      // the chunk's last M-step reports (a store to host memory costs an M-step ~1 us: not every one)
        HIPCHK(c, iterate(n));
        launched += n;
        if ((rc = mbox_done(launched - n, false, &stop))) return rc;
    }
    if (!stop && (rc = mbox_done(0, true, &stop))) return rc;      // the last chunk reaches max_iter, which ends the registration
    return take_mbox(false);
}

// early exit (trackdlo.cpp:424-428) is decided on the device; kernels of finished frames are
// no-ops.  To avoid enqueueing up to max_iter of them, iterations go out in chunks and the
// `done` flags of chunk i are inspected while chunk i+1 is already running (the GPU never idles).
int FramesCall::drive_polled() {
    IterState *flags = (IterState *)(c->pin + (size_t)F * nc.upload + fdd);     // pinned, 2 x F entries (one frame) ...
    double *fl_rb = c->pin + (size_t)F * nc.upload + fdd;                        // ... or 2 x F read-back blocks (batches)
    const double *results_dev = merged ? c->xfer + (size_t)F * up + fdd : nodeblk_used + nc.Yout;
    // A tracker in steady state converges in its first iteration (launch tolerance 2e-4): the first iteration is followed by the
    // read-back block itself (results + state) and a host sync; if every frame is done the call is over -- no second chunk of
    // no-op kernels, no separate flag copies (two no-op kernels and two 4 us copies per registration: 20 us of a 90 us call).
    HIPCHK(c, iterate(1));
    HIPCHK(c, join());
    if (timing) HIPCHK(c, hipEventRecord(c->ev[2], s));
    HIPCHK(c, hipMemcpyAsync(c->pin, results_dev, (size_t)F * nc.readback * sizeof(double), hipMemcpyDeviceToHost, s));
    if (timing) HIPCHK(c, hipEventRecord(c->ev[3], s));
    HIPCHK(c, wait_stream(s));
    have_readback = every_frame_done(c->pin, rstride(), nc, F);
    int launched = 1;
    bool stop = have_readback;
    for (int chunk = 0; launched < p->max_iter && !stop; ++chunk) {
        const int n = chunk_iters(chunk, p->max_iter - launched);
        HIPCHK(c, iterate(n));
        launched += n;
        const int slotp = chunk & 1;
        if (merged) {           // the whole read-back area (Yout + IterState per frame) in one copy, after the groups have joined
            HIPCHK(c, join());
            HIPCHK(c, hipMemcpyAsync(fl_rb + (size_t)slotp * F * nc.readback, results_dev, (size_t)F * nc.readback * sizeof(double), hipMemcpyDeviceToHost, s));
        } else {
            HIPCHK(c, hipMemcpyAsync(&flags[slotp], c->fh[0].st, sizeof(IterState), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(c, hipEventRecord(c->ev[4 + slotp], s));
        if (chunk > 0) {
            const int prev = (chunk - 1) & 1;
            HIPCHK(c, hipEventSynchronize(c->ev[4 + prev]));
            stop = merged ? every_frame_done(fl_rb + (size_t)prev * F * nc.readback, nc.readback, nc, F) : flags[prev].done != 0;
        }
    }
    return 0;
}

// the results into the staging buffer, unless the loop's driver has them there already
int FramesCall::read_back() {
    if (!have_readback) {
        HIPCHK(c, join());
        if (timing) HIPCHK(c, hipEventRecord(c->ev[2], s));
        // the upload block in pinned memory is consumed by now in stream order; reuse it for the readback
        if (merged) HIPCHK(c, hipMemcpyAsync(c->pin, c->xfer + (size_t)F * up + fdd, (size_t)F * nc.readback * sizeof(double), hipMemcpyDeviceToHost, s));
        else HIPCHK(c, hipMemcpyAsync(c->pin, nodeblk_used + nc.Yout, nc.readback * sizeof(double), hipMemcpyDeviceToHost, s));
        if (timing) HIPCHK(c, hipEventRecord(c->ev[3], s));
        HIPCHK(c, wait_stream(s));
    }
    c->last_F = F;
    return 0;
}

// The two verdicts after which the call is run again, once, another way -- inputs, Y and sigma2 are untouched so far.  true: *rc is the repeat's result.
bool FramesCall::repeat(int *rc) {
    auto drop_what_was_launched_ahead = [&] {
        if (c->pair.ahead) { spec_abort(c); c->pair.state = 0; c->pair.ahead = false; }      // (the repeat is another call: the main registration takes the ordinary route)
        else c->pair.spec = 0;             // (a paired M-step launched ahead has seen the error status and left)
    };
    // The banded L D L^T takes no pivots: a system that is not positive definite in floating point (an indefinite H_override; a chain the gap
    // test let through and rounding did not) ends its registration with TDLO_E_NUMERIC.  The reference's solver is a general one
    // (trackdlo.cpp:415), so the call is repeated once on the dense pivoted kernels and only their verdict is reported.
    if (p->include_lle && c->fh[0].lle_band && !c->lle_dense_once && any_frame_ended_with(TDLO_E_NUMERIC, c->pin, rstride(), nc, F)) {
        drop_what_was_launched_ahead();
        c->lle_dense_once = true;
        ++c->band_retries;
        *rc = run_frames(c, F, slots, Y, M, sigma2, p, nullptr, 0, nullptr, 0, nullptr, stats, nullptr, fa.data());
        c->lle_dense_once = false;
        return true;
    }
    // fp64 mode: the E-step's range check runs against limits that follow sigma (IterState::sh_boost: finer sums while sigma is small).  The extent
    // behind them is a heuristic (D_eff = 2 (0.4 m + 2 sigma)): a registration whose shares exceed it -- nodes dragged far by priors while sigma is
    // small -- would have passed under the coarse limits.  It is not failed for the boost: the call is repeated ONCE without it, and only that
    // verdict is reported.
    if (p->precision == TDLO_PREC_F64 && !c->boost_off_once && p->max_iter > 0 && any_frame_ended_with(TDLO_E_NUMERIC, c->pin, rstride(), nc, F)) {
        drop_what_was_launched_ahead();
        c->boost_off_once = true;
        ++c->boost_retries;
        for (int i = 0; i < F; ++i) c->slots[slots[i]].sorted_valid = false;
        *rc = run_frames(c, F, slots, Y, M, sigma2, p, nullptr, 0, nullptr, 0, nullptr, stats, late, fa.data());      // (late priors: formed again from the same guide nodes)
        c->boost_off_once = false;
        return true;
    }
    return false;
}

// nodes, sigma2 and statistics to the caller; the call's verdict
int FramesCall::results_out(std::chrono::steady_clock::time_point t_host0) {
    float loop_ms = 0, total_ms = 0;
    if (timing) { hipEventElapsedTime(&loop_ms, c->ev[1], c->ev[2]); hipEventElapsedTime(&total_ms, c->ev[0], c->ev[3]); }
    const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
    int worst = 0;
    for (int i = 0; i < F; ++i) {
        const double *rb = c->pin + (size_t)i * rstride();
        IterState is = readback_state(c->pin, rstride(), nc, i);
        if (is.status == 0 || is.status == TDLO_E_NUMERIC) {
            if (p->max_iter > 0 && is.it > 0) std::memcpy(Y + (size_t)i * 3 * M, rb, sizeof(double) * 3 * M);
            sigma2[i] = is.sigma2;
        }
        if (lle_next && i == 0 && is.status == 0 && is.done != 0 && is.it > 0) {      // (the finishing M-step has formed H of exactly these nodes)
            Slot &sl = slot0();
            sl.hb_next_Y.assign(Y, Y + 3 * (size_t)M);
            sl.hb_next_valid = true;
        }
        if (p->max_iter == 0) { is.converged = 1; }
        if (stats) {
            fill_stats(&stats[i], is);
            stats[i].loop_ms = loop_ms; stats[i].total_ms = total_ms; stats[i].host_ms = host_ms;
            stats[i].sort_reused = ahead ? 0 : (paired ? 2 : c->fh[i].reuse_sorted); stats[i].band_retry = c->lle_dense_once ? 1 : 0;      // (ahead: its own prune and sort, in the twin slot)
        }
        if (is.status != 0 && worst == 0) worst = is.status;
    }
    g_prof.mark(g_prof.base + 6);
    {   // the measurement and debug entry points relaunch from these descriptors: nothing of this call's hand-overs may ride along (a stale mailbox
        // epoch, late priors copied again at it == 0, another registration's sums overwritten through pair_sums: ADVICE r04)
        FrameDev &f0 = c->fh[0];
        f0.lle_next = nullptr; f0.spec_flag = nullptr; f0.spec_prev = nullptr;
        f0.host_prog = nullptr; f0.host_out = nullptr; f0.host_epoch = 0; f0.host_report_it = 0;
        f0.late_aJ = nullptr; f0.late_aYd = nullptr; f0.late_mstep = 0; f0.pair_sums = nullptr; f0.Xhost = nullptr;
    }
    if (worst != 0 && !late && !c->pair.ahead) c->pair.spec = 0;      // (ahead: tracking_step tells the waiting M-step to leave)
    if (ahead) c->twin_busy = false;       // (what may still be on the second stream are no-op iterations on the twin slot's device buffers)
    if (worst == TDLO_E_FUSE) return TDLO_E_FUSE;      // the fused prologue's barrier was abandoned: the entry point repeats the call on the three-kernel route (fuse_fallback)
    if (worst == TDLO_E_EMPTY) return fail(c, worst, "every point was pruned (no point within 0.1 m of a node, trackdlo.cpp:190)");
    if (worst == TDLO_E_NUMERIC) return fail(c, worst, "non-finite or non-positive sigma2, or singular M-step system");
    return TDLO_OK;
}

// Shared driver of tdlo_cpd_lle_resident / _batch.
int run_frames(tdlo_ctx *c, int F, const int *slots, double *Y, int M, double *sigma2, const tdlo_params *p,
               const double *priors, int K, const int *vis, int n_vis, const double *H_override, tdlo_stats *stats,
               const LatePriors *late, const tdlo_frame_args *each) {
    const auto t_host0 = std::chrono::steady_clock::now();
    int rc = check_params(c, M, p);
    if (rc) return rc;
    const int iter_hint = c->iter_hint_on ? c->iter_hint : 0;
    if (!c->iter_hint_on) c->iter_hint_next = 0;
    c->iter_hint = 0;
    if (late && F != 1) return fail(c, TDLO_E_INVALID, "late priors: one frame per call");
    if (F < 1 || F > c->cfg.max_frames) return fail(c, TDLO_E_INVALID, "bad frame count");
    FramesCall k(c, F, slots, Y, M, sigma2, p, priors, K, vis, n_vis, H_override, stats, late, iter_hint, each);
    if ((rc = k.size_staging())) return rc;             // the pinned staging buffer, a batch's transfer buffer
    k.recognise_pair();                                 // tracking_step's second registration, set up (or begun) by the first one's call
    if ((rc = k.stage_frames())) return rc;             // upload blocks and descriptors; a batch's kernels
    if ((rc = k.choose_routes())) return rc;            // tracking_step's short cuts; late priors that cannot wait; the sort reused per launch
    if ((rc = k.open_mailbox())) return rc;             // one frame on a one-workgroup M-step reports through pinned host memory
    if ((rc = k.upload_and_prologue())) return rc;      // blocks to the device; prune, sort, set-up
    if ((rc = k.stage_late_priors())) return rc;        // priors formed beside the set-up kernel
    if ((rc = k.fork_streams())) return rc;             // a batch's stream groups
    k.choose_loop();                                    // how the first iteration starts; one launch per iteration or two
    if (k.fixed_count()) rc = k.drive_fixed();          // the EM loop: everything enqueued up front,
    else if (k.use_mbox) rc = k.drive_mailbox();        // ... early exit read from the mailbox,
    else rc = k.drive_polled();                         // ... or polled by copies of the frames' state
    if (rc) return rc;
    if ((rc = k.read_back())) return rc;                // results into the staging buffer
    if (k.repeat(&rc)) return rc;                       // banded solve -> dense kernels; fp64 sums without the boost
    return k.results_out(t_host0);
}

// dst[c * N + n] = (D)src[n * stride_point + c * stride_comp]: the one pass over a host view's points (D = S: packed in the source precision for
// the import kernel; D = double: widened straight into a small tracker frame's staging)
template <typename D, typename S>
void view_gather(D *dst, const S *src, long long sp, long long sc, int N) {
    D *x = dst, *y = dst + (size_t)N, *z = dst + 2 * (size_t)N;
    for (long long n = 0; n < N; ++n) {
        const S *p = src + n * sp;
        x[n] = (D)p[0]; y[n] = (D)p[sc]; z[n] = (D)p[2 * sc];
    }
}

}  // namespace

// =================================================================================================
extern "C" {

int tdlo_abi_version(void) { return TDLO_ABI_VERSION; }

int tdlo_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void tdlo_default_config(tdlo_config *cfg) {
    if (!cfg) return;
    cfg->device = 0; cfg->max_frames = 1; cfg->max_points = 65536; cfg->max_nodes = 64; cfg->estep_blocks = 0;
}

tdlo_ctx *tdlo_create(const tdlo_config *cfg_in, int *err) {
    tdlo_config cfg;
    if (cfg_in) cfg = *cfg_in; else tdlo_default_config(&cfg);
    auto bail = [&](int code) -> tdlo_ctx * { if (err) *err = code; return nullptr; };
    int n = 0;
    hipError_t he = hipGetDeviceCount(&n);
    if (he != hipSuccess || n <= 0 || cfg.device < 0 || cfg.device >= n) {
        fprintf(stderr, "trackdlo_hip: hipGetDeviceCount -> %s, %d device(s), requested %d\n", hipGetErrorString(he), n, cfg.device);
        return bail(TDLO_E_NO_DEVICE);
    }
    he = hipSetDevice(cfg.device);
    if (he != hipSuccess) { fprintf(stderr, "trackdlo_hip: hipSetDevice -> %s\n", hipGetErrorString(he)); return bail(TDLO_E_NO_DEVICE); }
    if (check_device_image() != 0) return bail(TDLO_E_NO_DEVICE);     // no gfx950 code object for this device
    if (cfg.max_frames < 1) cfg.max_frames = 1;
    tdlo_ctx *c = new tdlo_ctx();
    c->device = cfg.device; c->cfg = cfg;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return bail(TDLO_E_HIP); }
    for (auto &e : c->ev) if (hipEventCreate(&e) != hipSuccess) { delete c; return bail(TDLO_E_HIP); }
    for (auto &e : c->evx) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { delete c; return bail(TDLO_E_HIP); }
    for (auto &e : c->evj) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { delete c; return bail(TDLO_E_HIP); }
    c->slots.resize(cfg.max_frames);
    if (hipMalloc((void **)&c->fd, sizeof(FrameDev) * cfg.max_frames) != hipSuccess) { delete c; return bail(TDLO_E_HIP); }
    for (auto &s : c->slots) {
        if (ensure_points(c, s, std::max(cfg.max_points, 1024)) || ensure_nodes(c, s, std::max(cfg.max_nodes, 16))) {
            if (err) *err = TDLO_E_HIP;
            tdlo_destroy(c);
            return nullptr;
        }
    }
    if (err) *err = TDLO_OK;
    return c;
}

void tdlo_destroy(tdlo_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (auto &q : c->stream2) if (q) hipStreamSynchronize(q);
    c->slots.push_back(c->twin);          // (freed with the others)
    for (auto &s : c->slots) {
        if (s.Xraw) hipFree(s.Xraw);
        if (s.Xs) hipFree(s.Xs);
        if (s.bucket) hipFree(s.bucket);
        if (s.blksum) hipFree(s.blksum);
        if (s.hist) hipFree(s.hist);
        if (s.nodeblk) hipFree(s.nodeblk);
        if (s.nodeblk2) hipFree(s.nodeblk2);
        if (s.hb_next) hipFree(s.hb_next);
        if (s.sync) hipFree(s.sync);
    }
    delete c->pool; c->pool = nullptr;
    if (c->fd) hipFree(c->fd);
    if (c->cloud_ws) hipFree(c->cloud_ws);
    if (c->cloud_fws) hipFree(c->cloud_fws);
    if (c->cbat_dev) hipFree(c->cbat_dev);
    if (c->cbat_img) hipFree(c->cbat_img);
    if (c->cbat_pin) hipHostFree(c->cbat_pin);
    if (c->wbat_dev) hipFree(c->wbat_dev);
    if (c->wbat_pin) hipHostFree(c->wbat_pin);
    if (c->rbatch_dev) hipFree(c->rbatch_dev);
    if (c->rbatch_pin) hipHostFree(c->rbatch_pin);
    if (c->pnt_dev) hipFree(c->pnt_dev);
    if (c->pnt_pin) hipHostFree(c->pnt_pin);
    if (c->cel_dev) hipFree(c->cel_dev);
    if (c->cel_pin) hipHostFree(c->cel_pin);
    if (c->asg_dev) hipFree(c->asg_dev);
    if (c->asg_state) hipFree(c->asg_state);
    if (c->asg_res) hipHostFree(c->asg_res);
    if (c->aln_dev) hipFree(c->aln_dev);
    if (c->aln_pin) hipHostFree(c->aln_pin);
    if (c->aln_res) hipHostFree(c->aln_res);
    if (c->alnb_dev) hipFree(c->alnb_dev);
    if (c->alnb_up) hipFree(c->alnb_up);
    if (c->alnb_pin) hipHostFree(c->alnb_pin);
    if (c->alnb_ev_up) hipEventDestroy(c->alnb_ev_up);
    for (hipEvent_t e : c->alnb_ev) hipEventDestroy(e);
    for (hipEvent_t e : c->wbat_ev) hipEventDestroy(e);
    if (c->vis_state) hipFree(c->vis_state);
    if (c->vis_res) hipHostFree(c->vis_res);
    if (c->vis_nodes_pin) hipHostFree(c->vis_nodes_pin);
    if (c->vbat_state) hipFree(c->vbat_state);
    if (c->vbat_res) hipHostFree(c->vbat_res);
    if (c->cloud_res) hipHostFree(c->cloud_res);
    if (c->img_pin) hipHostFree(c->img_pin);
    if (c->col_pin) hipHostFree(c->col_pin);
    if (c->col_dev) hipFree(c->col_dev);
    if (c->res_pin) hipHostFree(c->res_pin);
    if (c->res_dev) hipFree(c->res_dev);
    if (c->rnd_pin) hipHostFree(c->rnd_pin);
    if (c->rnd_dev) hipFree(c->rnd_dev);
    if (c->rbat_pin) hipHostFree(c->rbat_pin);
    if (c->rbat_dev) hipFree(c->rbat_dev);
    if (c->reg_ws) hipFree(c->reg_ws);
    if (c->pin) hipHostFree(c->pin);
    if (c->pin2) hipHostFree(c->pin2);
    if (c->cloud_pin) hipHostFree(c->cloud_pin);
    if (c->mbox) hipHostFree(c->mbox);
    if (c->late_buf) hipHostFree(c->late_buf);
    for (auto &e : c->ev) if (e) hipEventDestroy(e);
    if (c->xfer) hipFree(c->xfer);
    if (c->split_buf) hipFree(c->split_buf);
    for (void *p : c->xch_opened) hipIpcCloseMemHandle(p);
    if (c->xch_own) hipFree(c->xch_own);
    if (c->own_comm) { const RcclApi *r = rccl_api(nullptr, nullptr); if (r) r->CommDestroy(c->own_comm); }
    for (auto &e : c->evx) if (e) hipEventDestroy(e);
    for (auto &e : c->evj) if (e) hipEventDestroy(e);
    if (c->ev_view) hipEventDestroy(c->ev_view);
    for (auto &q : c->stream2) if (q) hipStreamDestroy(q);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

const char *tdlo_last_error(const tdlo_ctx *c) { return c ? c->err.c_str() : "no context (no usable HIP device?)"; }
void *tdlo_stream(tdlo_ctx *c) { return c ? (void *)c->stream : nullptr; }

int tdlo_synchronize(tdlo_ctx *c) {
    if (!c) return TDLO_E_INVALID;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TDLO_OK;
}

// sync == false: the copy is only enqueued -- for callers that keep X alive until their next synchronisation with the stream
// (tracking_step: the first registration's read-back waits for everything before it)
static int set_cloud_impl(tdlo_ctx *c, int slot, const double *X, int N, bool sync) {
    if (!c) return TDLO_E_INVALID;
    if (slot < 0 || slot >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
    if (!X || N <= 0) return fail(c, TDLO_E_INVALID, "empty cloud");
    HIPCHK(c, hipSetDevice(c->device));
    Slot &s = c->slots[slot];
    int rc = ensure_points(c, s, N);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(s.Xraw, X, 3 * (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (sync) HIPCHK(c, wait_stream(c->stream));      // caller may free X on return (by-value semantics)
    s.N0 = N; s.sorted_valid = false;
    return TDLO_OK;
}

int tdlo_set_cloud(tdlo_ctx *c, int slot, const double *X, int N) { return set_cloud_impl(c, slot, X, N, true); }

// ---- cloud views: float32 / float64, any strides, host or device memory --------------------------------------------------------------------------
// lowest and highest element offset the view addresses (n * stride_point + c * stride_comp over n < N, c < 3), in 128 bits: a stride is any long long
static void view_span(const tdlo_cloud_view *v, int N, __int128 *lo, __int128 *hi) {
    const __int128 a = (__int128)(N - 1) * v->stride_point, b = (__int128)2 * v->stride_comp;
    *lo = (a < 0 ? a : 0) + (b < 0 ? b : 0);
    *hi = (a > 0 ? a : 0) + (b > 0 ? b : 0);
}

// nullptr: (v, N) describes a cloud; otherwise what is wrong with it
static const char *view_fault(const tdlo_cloud_view *v, int N) {
    if (!v) return "cloud view: null view";
    if (!v->data) return "cloud view: null data";
    if (N <= 0) return "cloud view: empty cloud";
    if (v->dtype != TDLO_F32 && v->dtype != TDLO_F64) return "cloud view: unknown dtype";
    if (v->location != TDLO_MEM_AUTO && v->location != TDLO_MEM_HOST && v->location != TDLO_MEM_DEVICE) return "cloud view: unknown location";
    if (v->flags & ~TDLO_VIEW_ASYNC) return "cloud view: unknown flag";
    if (v->stride_point == 0 && N > 1) return "cloud view: stride_point is 0";
    if (v->stride_comp == 0) return "cloud view: stride_comp is 0";
    const int es = v->dtype == TDLO_F32 ? 4 : 8;
    if ((uintptr_t)v->data % (uintptr_t)es) return "cloud view: data is not aligned to its element size";
    __int128 lo, hi;
    view_span(v, N, &lo, &hi);
    const __int128 lim = (__int128)1 << 62;
    if (lo * es <= -lim || (hi + 1) * es >= lim) return "cloud view: the extent does not fit 64-bit byte offsets";
    return nullptr;
}

int tdlo_cloud_view_check(const tdlo_cloud_view *v, int N) { return view_fault(v, N) ? TDLO_E_INVALID : TDLO_OK; }

int tdlo_cloud_view_extent(const tdlo_cloud_view *v, int N, long long *lo_bytes, long long *hi_bytes) {
    if (view_fault(v, N) || !lo_bytes || !hi_bytes) return TDLO_E_INVALID;
    const int es = v->dtype == TDLO_F32 ? 4 : 8;
    __int128 lo, hi;
    view_span(v, N, &lo, &hi);
    *lo_bytes = (long long)(lo * es); *hi_bytes = (long long)((hi + 1) * es);
    return TDLO_OK;
}

// Where a (checked) view's memory is: *device = a kernel on the context's GPU may read it.  Everything else -- memory the runtime does not know,
// caller-pinned and managed memory -- is host memory: copied, never dereferenced by a kernel.
static int pointer_location(tdlo_ctx *c, const void *data, int location, const char *what, bool *device) {
    *device = false;
    if (location == TDLO_MEM_HOST) return TDLO_OK;
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, data) != hipSuccess) {
        (void)hipGetLastError();                           // (a pointer the runtime does not know; the error must not reach the next launch check)
        if (location == TDLO_MEM_DEVICE) return fail(c, TDLO_E_INVALID, std::string(what) + ": location says device memory, the runtime does not know the pointer");
        return TDLO_OK;
    }
    if (at.type != hipMemoryTypeDevice) {
        if (location == TDLO_MEM_DEVICE) return fail(c, TDLO_E_INVALID, std::string(what) + ": location says device memory, the runtime says otherwise");
        return TDLO_OK;
    }
    if (at.device != c->device) return fail(c, TDLO_E_INVALID, std::string(what) + ": device memory of another GPU");
    *device = true;
    return TDLO_OK;
}
static int view_location(tdlo_ctx *c, const tdlo_cloud_view *v, bool *device) { return pointer_location(c, v->data, v->location, "cloud view", device); }

// tdlo_set_cloud_view on a checked view.  wait: the call returns when the import has finished (a host source always waits unless the caller is
// tracking_step, whose first registration waits for the stream before it returns: the pinned staging is free again by then).
static int import_view(tdlo_ctx *c, int slot, const tdlo_cloud_view *v, int N, bool device, bool wait) {
    Slot &s = c->slots[slot];
    int rc;
    if ((rc = flush_pending_cloud(c)) || (rc = ensure_points(c, s, N))) return rc;
    const bool f64 = v->dtype == TDLO_F64;
    if (device) {
        if (v->ready_stream) {
            if (!c->ev_view) HIPCHK(c, hipEventCreateWithFlags(&c->ev_view, hipEventDisableTiming));
            HIPCHK(c, hipEventRecord(c->ev_view, (hipStream_t)v->ready_stream));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_view, 0));
        }
        HIPCHK(c, launch_cloud_import(v->data, f64, v->stride_point, v->stride_comp, N, s.Xraw, c->stream));
    } else {
        const size_t bytes = 3 * (size_t)N * (f64 ? 8 : 4);
        if ((rc = ensure_cloud_pin(c, (bytes + 7) / 8))) return rc;
        if (f64) view_gather((double *)c->cloud_pin, (const double *)v->data, v->stride_point, v->stride_comp, N);
        else view_gather((float *)c->cloud_pin, (const float *)v->data, v->stride_point, v->stride_comp, N);
        const void *src = c->cloud_pin;
        if (!c->view_inplace) {
            HIPCHK(c, hipMemcpyAsync(s.Xs, c->cloud_pin, bytes, hipMemcpyHostToDevice, c->stream));
            src = s.Xs;
        }
        HIPCHK(c, launch_cloud_import(src, f64, 1, N, N, s.Xraw, c->stream));
    }
    s.N0 = N; s.sorted_valid = false;
    ++c->view_route[0];
    if (wait) HIPCHK(c, wait_stream(c->stream));
    return TDLO_OK;
}

int tdlo_set_cloud_view(tdlo_ctx *c, int slot, const tdlo_cloud_view *v, int N) {
    if (!c) return TDLO_E_INVALID;
    if (const char *why = view_fault(v, N)) return fail(c, TDLO_E_INVALID, why);
    if (slot < 0 || slot >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
    HIPCHK(c, hipSetDevice(c->device));
    bool device = false;
    if (int rc = view_location(c, v, &device)) return rc;
    return import_view(c, slot, v, N, device, !(device && (v->flags & TDLO_VIEW_ASYNC)));
}

int tdlo_get_cloud(tdlo_ctx *c, int slot, double *X_out, int x_capacity, int *n_out) {
    if (!c) return TDLO_E_INVALID;
    if (slot < 0 || slot >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
    Slot &s = c->slots[slot];
    if (n_out) *n_out = s.N0;
    if (s.N0 > 0 && (!X_out || x_capacity < s.N0)) return fail(c, TDLO_E_INVALID, "tdlo_get_cloud: X_out is too small for the slot's cloud");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = flush_pending_cloud(c)) return rc;
    if (s.N0 > 0) HIPCHK(c, hipMemcpyAsync(X_out, s.Xraw, 3 * (size_t)s.N0 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, wait_stream(c->stream));
    return TDLO_OK;
}

// run_frames for the entry points that register caller-supplied nodes (tdlo_cpd_lle_resident, tdlo_cpd_lle_batch): a registration whose fused
// prologue was abandoned at its grid barrier (TDLO_E_FUSE: internal, no caller ever sees the code) has touched neither Y, sigma2 nor the slots'
// clouds -- the context is taken off the fused prologue (fuse_fallback: arrivals and barrier word reset, fuse_on = false) and the call repeated
// ONCE on the copy + three-kernel route.  (tracking_step's main registration does the same around its own call: it forms its priors again.)
static int run_frames_checked(tdlo_ctx *c, int F, const int *slots, double *Y, int M, double *sigma2, const tdlo_params *p,
                              const double *priors, int K, const int *vis, int n_vis, const double *H_override, tdlo_stats *stats,
                              const tdlo_frame_args *each = nullptr) {
    int rc = run_frames(c, F, slots, Y, M, sigma2, p, priors, K, vis, n_vis, H_override, stats, nullptr, each);
    if (rc == TDLO_E_FUSE) {
        fuse_fallback(c);
        rc = run_frames(c, F, slots, Y, M, sigma2, p, priors, K, vis, n_vis, H_override, stats, nullptr, each);
        if (rc == TDLO_E_FUSE) rc = fail(c, TDLO_E_HIP, "the fused prologue reported a time-out on the route that does not use it");
    }
    return rc;
}

int tdlo_cpd_lle_resident(tdlo_ctx *c, int slot, double *Y, int M, double *sigma2, const tdlo_params *p,
                          const double *priors, int K, const int *vis, int n_vis, const double *H_override,
                          tdlo_stats *stats) {
    if (!c) return TDLO_E_INVALID;
    if (slot < 0 || slot >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
    if (!Y || !sigma2) return fail(c, TDLO_E_INVALID, "null Y / sigma2");
    HIPCHK(c, hipSetDevice(c->device));
    return run_frames_checked(c, 1, &slot, Y, M, sigma2, p, priors, K, vis, n_vis, H_override, stats);
}

int tdlo_cpd_lle(tdlo_ctx *c, const double *X, int N, double *Y, int M, double *sigma2, const tdlo_params *p,
                 const double *priors, int K, const int *vis, int n_vis, const double *H_override, tdlo_stats *stats) {
    int rc = tdlo_set_cloud(c, 0, X, N);
    if (rc) return rc;
    return tdlo_cpd_lle_resident(c, 0, Y, M, sigma2, p, priors, K, vis, n_vis, H_override, stats);
}

int tdlo_cpd_lle_batch(tdlo_ctx *c, int F, double *Y, int M, double *sigma2, const tdlo_params *p,
                       const double *priors, int K, const int *vis, int n_vis, const double *H_override,
                       tdlo_stats *stats) {
    if (!c) return TDLO_E_INVALID;
    if (F < 1 || F > (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad frame count");
    if (!Y || !sigma2) return fail(c, TDLO_E_INVALID, "null Y / sigma2");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int> slots(F);
    for (int i = 0; i < F; ++i) slots[i] = i;
    return run_frames_checked(c, F, slots.data(), Y, M, sigma2, p, priors, K, vis, n_vis, H_override, stats);      // (F == 1 takes the fused prologue like a single call)
}

// A batch whose frames bring their own priors, visible sets and H (args == NULL: none).  One frame is the one-frame route.  The E-step kernels
// are instantiated per launch with or without the visibility weights (FrameDev::vis_branch), so frames that disagree there run as two batches, one behind the
// other -- independent registrations: the results do not depend on the split.  Every frame's statistics are filled; returns the first non-zero code.
static int run_frames_each(tdlo_ctx *c, int F, const int *slots, double *Y, int M, double *sigma2, const tdlo_params *p, const tdlo_frame_args *args, tdlo_stats *stats) {
    if (F == 1) {
        const tdlo_frame_args a = args ? args[0] : tdlo_frame_args{nullptr, 0, nullptr, 0, nullptr};
        return run_frames_checked(c, 1, slots, Y, M, sigma2, p, a.priors, a.K, a.visible_nodes, a.n_vis, a.H_override, stats);
    }
    if (!p) return fail(c, TDLO_E_INVALID, "params is null");
    std::vector<tdlo_frame_args> none;
    if (!args) { none.assign(F, tdlo_frame_args{nullptr, 0, nullptr, 0, nullptr}); args = none.data(); }
    std::vector<int> grp[2];
    for (int i = 0; i < F; ++i) grp[frame_vis_branch(args[i].n_vis, M, p) ? 1 : 0].push_back(i);
    if (grp[0].empty() || grp[1].empty()) return run_frames_checked(c, F, slots, Y, M, sigma2, p, nullptr, 0, nullptr, 0, nullptr, stats, args);
    int first = 0;
    for (const std::vector<int> &g : grp) {
        const int Fg = (int)g.size();
        std::vector<int> sl(Fg); std::vector<double> Yg(3 * (size_t)M * Fg), s2(Fg); std::vector<tdlo_frame_args> ag(Fg); std::vector<tdlo_stats> sg(Fg);
        for (int k = 0; k < Fg; ++k) {
            const int i = g[k];
            sl[k] = slots[i]; s2[k] = sigma2[i]; ag[k] = args[i];
            std::memcpy(&Yg[3 * (size_t)M * k], Y + 3 * (size_t)M * i, sizeof(double) * 3 * M);
        }
        const int rc = run_frames_each(c, Fg, sl.data(), Yg.data(), M, s2.data(), p, ag.data(), sg.data());
        for (int k = 0; k < Fg; ++k) {
            const int i = g[k];
            sigma2[i] = s2[k];
            std::memcpy(Y + 3 * (size_t)M * i, &Yg[3 * (size_t)M * k], sizeof(double) * 3 * M);
            if (stats) stats[i] = sg[k];
        }
        if (rc && !first) first = rc;
    }
    return first;
}

int tdlo_cpd_lle_batch_each(tdlo_ctx *c, int F, const int *slots, double *Y, int M, double *sigma2, const tdlo_params *p,
                            const tdlo_frame_args *args, tdlo_stats *stats) {
    if (!c) return TDLO_E_INVALID;
    if (F < 1 || F > (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad frame count");
    if (!Y || !sigma2) return fail(c, TDLO_E_INVALID, "null Y / sigma2");
    std::vector<int> own(F);
    for (int i = 0; i < F; ++i) {
        own[i] = slots ? slots[i] : i;
        if (own[i] < 0 || own[i] >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
        for (int j = 0; j < i; ++j) if (own[j] == own[i]) return fail(c, TDLO_E_INVALID, "the slots of a batch must be distinct");
    }
    HIPCHK(c, hipSetDevice(c->device));
    return run_frames_each(c, F, own.data(), Y, M, sigma2, p, args, stats);
}

// ---- N-split -------------------------------------------------------------------------------------
int tdlo_split_begin(tdlo_ctx *c, const double *Y, int M, double sigma2, const tdlo_params *p,
                     const double *priors, int K, const int *vis, int n_vis, const double *H_override, double *init) {
    if (!c) return TDLO_E_INVALID;
    int rc = check_params(c, M, p);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    NodeCarve nc(M);
    rc = ensure_pin(c, std::max(nc.upload, nc.readback + 2) + 8 * (size_t)M + 16);
    if (rc) return rc;
    c->fh.assign(1, FrameDev{});
    rc = prepare_frame(c, 0, Y, M, sigma2, p, priors, K, vis, n_vis, H_override, c->pin, c->fh[0]);
    if (rc) return rc;
    c->fh[0].reuse_sorted = 0; c->slots[0].sorted_valid = false;      // a shard is pruned and sorted by the split's own setup
    if (c->xch_sums) c->fh[0].sums = c->xch_sums;       // the reduced sums are exported to / consumed from the caller's buffer
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->slots[0].nodeblk, c->pin, upload_doubles(nc, p, c->fh[0].lle_band != 0) * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->fd, c->fh.data(), sizeof(FrameDev), hipMemcpyHostToDevice, s));
    HIPCHK(c, launch_split_setup(c->fd, c->fh.data(), s));
    HIPCHK(c, hipMemcpyAsync(c->pin, c->slots[0].nodeblk + nc.st, sizeof(IterState), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    IterState is;
    std::memcpy(&is, c->pin, sizeof is);
    if (init) { init[0] = (double)is.N; init[1] = is.sum_d2; }
    c->split_active = 1;
    c->last_F = 1;
    return TDLO_OK;
}

int tdlo_split_set_global(tdlo_ctx *c, double n_kept_global, double sum_d2_global) {
    if (!c || !c->split_active) return TDLO_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_split_set_global(c->fd, n_kept_global, sum_d2_global, c->stream));
    return TDLO_OK;
}

int tdlo_split_dmin(tdlo_ctx *c, double *dmin_sq) {
    if (!c || !c->split_active) return TDLO_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const FrameDev &f = c->fh[0];
    const int M = f.M;
    if (!f.vis_branch) { for (int m = 0; m < M; ++m) dmin_sq[m] = 0; return TDLO_OK; }
    hipStream_t s = c->stream;
    HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 1, s));
    HIPCHK(c, hipMemcpyAsync(c->pin, f.dminbits, sizeof(double) * M, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const unsigned long long *b = (const unsigned long long *)c->pin;
    for (int m = 0; m < M; ++m) {
        if (b[m] == ~0ull) { dmin_sq[m] = 1e300; continue; }
        if (f.precision == TDLO_PREC_F64) { double v; std::memcpy(&v, &b[m], 8); dmin_sq[m] = v; }
        else { unsigned u = (unsigned)b[m]; float v; std::memcpy(&v, &u, 4); dmin_sq[m] = (double)v; }
    }
    return TDLO_OK;
}

int tdlo_split_estep(tdlo_ctx *c, const double *dmin_sq_global, double *sums) {
    if (!c || !c->split_active) return TDLO_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const FrameDev &f = c->fh[0];
    const int M = f.M;
    hipStream_t s = c->stream;
    if (f.vis_branch && dmin_sq_global) {
        unsigned long long *b = (unsigned long long *)c->pin;
        for (int m = 0; m < M; ++m) {
            if (f.precision == TDLO_PREC_F64) { double v = dmin_sq_global[m]; std::memcpy(&b[m], &v, 8); }
            else { float v = (float)dmin_sq_global[m]; unsigned u; std::memcpy(&u, &v, 4); b[m] = u; }
        }
        HIPCHK(c, hipMemcpyAsync(f.dminbits, c->pin, sizeof(double) * M, hipMemcpyHostToDevice, s));
    }
    HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 0, s));
    HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 3, s));        // the shard's accumulators -> sums
    HIPCHK(c, hipMemcpyAsync(c->pin + M, f.sums, sizeof(double) * (4 * M + 2), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    std::memcpy(sums, c->pin + M, sizeof(double) * (4 * M + 2));
    return TDLO_OK;
}

int tdlo_split_mstep(tdlo_ctx *c, const double *sums_global, int *done) {
    if (!c || !c->split_active) return TDLO_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const FrameDev &f = c->fh[0];
    const int M = f.M;
    hipStream_t s = c->stream;
    std::memcpy(c->pin, sums_global, sizeof(double) * (4 * M + 2));
    HIPCHK(c, hipMemcpyAsync(f.sums, c->pin, sizeof(double) * (4 * M + 2), hipMemcpyHostToDevice, s));
    HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 4, s));
    HIPCHK(c, hipMemcpyAsync(c->pin + 4 * M + 4, f.st, sizeof(IterState), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    IterState is;
    std::memcpy(&is, c->pin + 4 * M + 4, sizeof is);
    if (done) *done = is.done;
    return TDLO_OK;
}

// Device-resident exchange: nothing below synchronises with the host except tdlo_split_poll.
int tdlo_split_bind_exchange(tdlo_ctx *c, double *d_dmin, double *d_sums) {
    if (!c) return TDLO_E_INVALID;
    if (c->split_active) return fail(c, TDLO_E_INVALID, "tdlo_split_bind_exchange inside a split registration");
    if ((d_dmin == nullptr) != (d_sums == nullptr)) return fail(c, TDLO_E_INVALID, "bind both exchange buffers or neither");
    c->xch_dmin = d_dmin; c->xch_sums = d_sums;
    return TDLO_OK;
}

int tdlo_split_dmin_enqueue(tdlo_ctx *c) {
    if (!c || !c->split_active) return TDLO_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->xch_dmin) return fail(c, TDLO_E_INVALID, "no exchange buffers bound");
    if (!c->fh[0].vis_branch) return TDLO_OK;
    HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 1, c->stream));
    HIPCHK(c, launch_split_dmin_xch(c->fd, c->fh.data(), c->xch_dmin, 0, c->stream));
    return TDLO_OK;
}

int tdlo_split_estep_enqueue(tdlo_ctx *c) {
    if (!c || !c->split_active) return TDLO_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->xch_sums) return fail(c, TDLO_E_INVALID, "no exchange buffers bound");
    hipStream_t s = c->stream;
    if (c->fh[0].vis_branch) HIPCHK(c, launch_split_dmin_xch(c->fd, c->fh.data(), c->xch_dmin, 1, s));
    HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 0, s));
    HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 3, s));        // the shard's accumulators -> the bound sums buffer
    return TDLO_OK;
}

int tdlo_split_mstep_enqueue(tdlo_ctx *c) {
    if (!c || !c->split_active) return TDLO_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->xch_sums) return fail(c, TDLO_E_INVALID, "no exchange buffers bound");
    HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 4, c->stream));
    return TDLO_OK;
}

int tdlo_split_poll(tdlo_ctx *c, int *done, int *iters) {
    if (!c || !c->split_active) return TDLO_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->pin, c->fh[0].st, sizeof(IterState), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    IterState is;
    std::memcpy(&is, c->pin, sizeof is);
    if (done) *done = is.done;
    if (iters) *iters = is.it;
    return TDLO_OK;
}

int tdlo_split_end(tdlo_ctx *c, double *Y, double *sigma2, tdlo_stats *stats) {
    if (!c || !c->split_active) return TDLO_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const FrameDev &f = c->fh[0];
    const int M = f.M;
    NodeCarve nc(M);
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->pin, c->slots[0].nodeblk + nc.Yout, nc.readback * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    IterState is;
    std::memcpy(&is, c->pin + (nc.st - nc.Yout), sizeof is);
    if (Y && is.it > 0) std::memcpy(Y, c->pin, sizeof(double) * 3 * M);
    if (sigma2) *sigma2 = is.sigma2;
    if (stats) { std::memset(stats, 0, sizeof *stats); fill_stats(stats, is); }
    c->split_active = 0;
    return is.status;
}

int tdlo_split_abort(tdlo_ctx *c) {
    if (!c) return TDLO_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->split_active = 0;
    c->xch_dmin = nullptr; c->xch_sums = nullptr;
    return TDLO_OK;
}

// ---- tdlo_split_run: the split registration driven from C++ ---------------------------------------------------------
int tdlo_rccl_load(const char *path) {
    std::string why;
    return rccl_api(path, &why) ? TDLO_OK : TDLO_E_EXCHANGE;
}

int tdlo_rccl_unique_id(void *id128) {
    std::string why;
    const RcclApi *r = rccl_api(nullptr, &why);
    if (!r || !id128) return TDLO_E_EXCHANGE;
    RcclApi::UniqueId id;
    if (r->GetUniqueId(&id) != 0) return TDLO_E_EXCHANGE;
    std::memcpy(id128, &id, sizeof id);
    return TDLO_OK;
}

int tdlo_rccl_comm_init(tdlo_ctx *c, int nranks, int rank, const void *id128, void **comm_out) {
    if (!c || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return TDLO_E_INVALID;
    std::string why;
    const RcclApi *r = rccl_api(nullptr, &why);
    if (!r) return fail(c, TDLO_E_EXCHANGE, "RCCL cannot be loaded: " + why);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->own_comm) { r->CommDestroy(c->own_comm); c->own_comm = nullptr; }
    RcclApi::UniqueId id;
    std::memcpy(&id, id128, sizeof id);
    void *comm = nullptr;
    const int rc = r->CommInitRank(&comm, nranks, id, rank);
    if (rc != 0) return fail(c, TDLO_E_EXCHANGE, std::string("ncclCommInitRank: ") + r->GetErrorString(rc));
    c->own_comm = comm;
    if (comm_out) *comm_out = comm;
    return TDLO_OK;
}

int tdlo_rccl_comm_count(void *comm, int *nranks, int *rank) {
    std::string why;
    const RcclApi *r = rccl_api(nullptr, &why);
    if (!r || !comm || !r->CommCount || !r->CommUserRank) return TDLO_E_EXCHANGE;
    int n = 0, me = 0;
    if (r->CommCount(comm, &n) != 0 || r->CommUserRank(comm, &me) != 0) return TDLO_E_EXCHANGE;
    if (nranks) *nranks = n;
    if (rank) *rank = me;
    return TDLO_OK;
}

size_t tdlo_xch_bytes(int nranks, int max_nodes) {
    if (nranks < 1 || nranks > kMaxXchRanks || max_nodes < 4) return 0;
    return xch_words(nranks, max_nodes) * sizeof(unsigned long long);
}

int tdlo_xch_create(tdlo_ctx *c, int nranks, int max_nodes, void **inbox) {
    if (!c) return TDLO_E_INVALID;
    if (nranks < 1 || nranks > kMaxXchRanks || max_nodes < 4 || max_nodes > kChainLdsMaxNodes) return fail(c, TDLO_E_INVALID, "tdlo_xch_create: 1..8 ranks, 4..512 nodes (longer chains: tdlo_split_run with an RCCL communicator)");
    if (c->split_active) return fail(c, TDLO_E_INVALID, "tdlo_xch_create inside a split registration");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->xch_own) { hipFree(c->xch_own); c->xch_own = nullptr; }
    c->xch_nranks = 0;
    const size_t words = xch_words(nranks, max_nodes);
    // peers write this buffer over xGMI while this GPU polls it: it must be uncached (fine-grained) device memory -- a peer's stores to
    // coarse-grained memory are not guaranteed to become visible to a kernel that polls through its local L2, and every wait would then
    // run into its time limit.  Where the runtime does not offer it the exchange is refused (TDLO_E_EXCHANGE) so that callers take the
    // RCCL form instead; a single rank has no peers and may use any memory.
    void *p = nullptr;
    if (hipExtMallocWithFlags(&p, words * sizeof(unsigned long long), hipDeviceMallocUncached) != hipSuccess) {
        (void)hipGetLastError();
        if (nranks > 1) return fail(c, TDLO_E_EXCHANGE, "tdlo_xch_create: no fine-grained (uncached) device memory for the inbox: use tdlo_split_run with an RCCL communicator");
        HIPCHK(c, hipMalloc(&p, words * sizeof(unsigned long long)));
    }
    HIPCHK(c, hipMemset(p, 0, words * sizeof(unsigned long long)));
    HIPCHK(c, hipDeviceSynchronize());
    c->xch_own = (unsigned long long *)p; c->xch_own_words = words; c->xch_mcap = max_nodes; c->xch_cap_ranks = nranks;
    if (inbox) *inbox = p;
    return TDLO_OK;
}

int tdlo_xch_ipc_export(tdlo_ctx *c, void *handle64) {
    if (!c || !handle64) return TDLO_E_INVALID;
    if (!c->xch_own) return fail(c, TDLO_E_INVALID, "tdlo_xch_ipc_export before tdlo_xch_create");
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t");
    HIPCHK(c, hipSetDevice(c->device));
    hipIpcMemHandle_t h;
    HIPCHK(c, hipIpcGetMemHandle(&h, c->xch_own));
    std::memcpy(handle64, &h, sizeof h);
    return TDLO_OK;
}

int tdlo_xch_ipc_open(tdlo_ctx *c, const void *handle64, void **peer_inbox) {
    if (!c || !handle64 || !peer_inbox) return TDLO_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle64, sizeof h);
    void *p = nullptr;
    {   // a GPU that cannot map the peer's memory is not a HIP failure of this library but a property of the node: TDLO_E_EXCHANGE, so that
        // every rank can fall back on the RCCL form together (bench.py: MIN over the ranks of "the exchange is set up")
        const hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, TDLO_E_EXCHANGE, std::string("tdlo_xch_ipc_open: the peer's inbox cannot be mapped on this GPU (") + hipGetErrorString(e) + ")"); }
    }
    c->xch_opened.push_back(p);
    *peer_inbox = p;
    return TDLO_OK;
}

int tdlo_xch_can_access(tdlo_ctx *c, int peer_device, int *can) {
    if (!c || !can) return TDLO_E_INVALID;
    *can = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || peer_device < 0 || peer_device >= n) return fail(c, TDLO_E_INVALID, "tdlo_xch_can_access: no such device");
    if (peer_device == c->device) { *can = 1; return TDLO_OK; }
    int ok = 0;
    HIPCHK(c, hipDeviceCanAccessPeer(&ok, c->device, peer_device));
    *can = ok;
    return TDLO_OK;
}

int tdlo_xch_bind(tdlo_ctx *c, int rank, int nranks, void *const *inboxes) {
    if (!c) return TDLO_E_INVALID;
    if (c->split_active) return fail(c, TDLO_E_INVALID, "tdlo_xch_bind inside a split registration");
    if (nranks == 0) { c->xch_nranks = 0; return TDLO_OK; }
    if (!c->xch_own || !inboxes || nranks != c->xch_cap_ranks || rank < 0 || rank >= nranks) return fail(c, TDLO_E_INVALID, "tdlo_xch_bind: create the inbox for this many ranks first");
    for (int r = 0; r < nranks; ++r) if (!inboxes[r]) return fail(c, TDLO_E_INVALID, "tdlo_xch_bind: null peer inbox");
    if (inboxes[rank] != (void *)c->xch_own) return fail(c, TDLO_E_INVALID, "tdlo_xch_bind: inboxes[rank] is not this context's own inbox");
    // inboxes of contexts of THIS process on other devices (one thread per GPU): plain device pointers -- this GPU must be able to map them
    HIPCHK(c, hipSetDevice(c->device));
    for (int r = 0; r < nranks; ++r) {
        if (r == rank) continue;
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, inboxes[r]) != hipSuccess) { (void)hipGetLastError(); continue; }      // (an IPC mapping: opened for this device already)
        if (at.device == c->device) continue;
        int ok = 0;
        HIPCHK(c, hipDeviceCanAccessPeer(&ok, c->device, at.device));
        if (!ok) return fail(c, TDLO_E_EXCHANGE, "tdlo_xch_bind: this GPU cannot access a peer's inbox (no peer mapping between the devices): use the RCCL form");
        const hipError_t e = hipDeviceEnablePeerAccess(at.device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(c, TDLO_E_EXCHANGE, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
        (void)hipGetLastError();
    }
    for (int r = 0; r < kMaxXchRanks; ++r) c->xch_peer[r] = r < nranks ? (unsigned long long *)inboxes[r] : nullptr;
    c->xch_rank = rank; c->xch_nranks = nranks;
    return TDLO_OK;
}

int tdlo_split_run(tdlo_ctx *c, void *nccl_comm, double *Y, int M, double *sigma2, const tdlo_params *p, const double *priors, int K,
                   const int *vis, int n_vis, const double *H_override, tdlo_stats *stats) {
    if (!c) return TDLO_E_INVALID;
    const auto t_host0 = std::chrono::steady_clock::now();
    if (!Y || !sigma2) return fail(c, TDLO_E_INVALID, "null Y / sigma2");
    if (c->split_active) return fail(c, TDLO_E_INVALID, "tdlo_split_run inside a split registration");
    int rc = check_params(c, M, p);
    if (rc) return rc;
    const bool oneshot = nccl_comm == nullptr;
    const RcclApi *R = nullptr;
    if (oneshot) {
        if (c->xch_nranks < 1) return fail(c, TDLO_E_INVALID, "tdlo_split_run without a communicator needs the one-shot exchange (tdlo_xch_create / tdlo_xch_bind)");
        if (M > c->xch_mcap) return fail(c, TDLO_E_INVALID, "more nodes than the inbox was created for");
    } else {
        std::string why;
        R = rccl_api(nullptr, &why);
        if (!R) return fail(c, TDLO_E_EXCHANGE, "RCCL cannot be loaded: " + why);
    }
    HIPCHK(c, hipSetDevice(c->device));
    NodeCarve nc(M);
    rc = ensure_pin(c, std::max(nc.upload, nc.readback + 2) + 8 * (size_t)M + 16);
    if (rc) return rc;
    c->fh.assign(1, FrameDev{});
    rc = prepare_frame(c, 0, Y, M, *sigma2, p, priors, K, vis, n_vis, H_override, c->pin, c->fh[0]);
    if (rc) return rc;
    c->fh[0].reuse_sorted = 0; c->slots[0].sorted_valid = false;      // a shard is pruned and sorted by the split's own setup
    FrameDev &f = c->fh[0];
    // the exchange lives in the one-workgroup M-steps: the chain smoother (no LLE term), the banded L D L^T (LLE term) -- any chain
    // length -- and the dense k_mstep_fast (up to 60 / 64 nodes)
    if (oneshot && M > kChainLdsMaxNodes)
        return fail(c, TDLO_E_INVALID, "the one-shot exchange serves chains of up to 512 nodes (the long-chain M-step does not carry it): pass an RCCL communicator");
    if (oneshot && !((!p->include_lle && (!f.mstep_dense || M <= 60)) || (p->include_lle && (f.lle_band || M <= 64))))
        return fail(c, TDLO_E_INVALID, "the one-shot exchange lives in the one-workgroup M-steps: this registration takes a dense multi-workgroup elimination (LLE term on a chain the banded solve cannot take, beyond 64 nodes): pass an RCCL communicator");
    hipStream_t s = c->stream;
    double *b_init = nullptr, *b_dmin = nullptr, *b_sums = nullptr;
    if (oneshot) {
        for (int r = 0; r < kMaxXchRanks; ++r) f.xch_inbox[r] = c->xch_peer[r];
        f.xch_rank = c->xch_rank; f.xch_nranks = c->xch_nranks; f.xch_mcap = c->xch_mcap; f.xch_epoch = ++c->xch_calls;
        f.xch_self = c->xch_self ? 1 : 0;          // a context setting (tdlo_set_xch_self; TDLO_XCH_SELF gives its initial value when the context is made)
        {   // test hook (tests/test_split_native_gpu.py): rank r's E-step refuses every sum as out of range -- an error of ONE shard, which its
            // peers must learn about inside the exchange (kXchErrMark) instead of waiting out the time limit
            static const int fail_rank = getenv("TDLO_TEST_RANGE_FAIL_RANK") ? atoi(getenv("TDLO_TEST_RANGE_FAIL_RANK")) : -1;
            if (fail_rank >= 0 && fail_rank == c->xch_rank) f.acc_lim[0] = f.acc_lim[1] = f.acc_lim[2] = 0.0;
        }
    } else {
        const size_t need = 2 + (size_t)M + 4 * (size_t)M + 2 + 2;
        if (need > c->split_buf_doubles) {
            HIPCHK(c, hipStreamSynchronize(s));
            if (c->split_buf) hipFree(c->split_buf);
            c->split_buf = nullptr; c->split_buf_doubles = 0;
            HIPCHK(c, hipMalloc((void **)&c->split_buf, need * sizeof(double)));
            c->split_buf_doubles = need;
        }
        b_init = c->split_buf; b_dmin = b_init + 2; b_sums = b_dmin + ((M + 1) & ~1);
        f.sums = b_sums;                                 // the export-only M-step writes, and the M-step from sums reads, this buffer
    }
    const bool timing = c->timing;
    if (timing) HIPCHK(c, hipEventRecord(c->ev[0], s));
    HIPCHK(c, hipMemcpyAsync(c->slots[0].nodeblk, c->pin, upload_doubles(nc, p, c->fh[0].lle_band != 0) * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->fd, c->fh.data(), sizeof(FrameDev), hipMemcpyHostToDevice, s));
    HIPCHK(c, launch_split_setup(c->fd, c->fh.data(), s));
    auto nccl = [&](int e, const char *what) -> int {
        if (e == 0) return 0;
        return fail(c, TDLO_E_EXCHANGE, std::string(what) + ": " + R->GetErrorString(e));
    };
    // once per call: kept points and the sigma2-initialisation sum over all shards (trackdlo.cpp:195, :263-273)
    if (oneshot) HIPCHK(c, launch_xch_init(c->fd, s));
    else {
        HIPCHK(c, launch_split_init_pack(c->fd, b_init, s));
        if ((rc = nccl(R->AllReduce(b_init, b_init, 2, kNcclFloat64, kNcclSum, nccl_comm, s), "ncclAllReduce(init)"))) return rc;
        HIPCHK(c, launch_split_set_global_dev(c->fd, b_init, s));
    }
    if (timing) HIPCHK(c, hipEventRecord(c->ev[1], s));
    const bool visb = f.vis_branch != 0;
    int split_it = 0;
    auto iteration = [&]() -> int {
        if (oneshot) {
            if (visb) HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 1, s));      // k_dmin: its last workgroup exchanges the minima
            HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 0, s));
            mstep_parity_hint(split_it++);                                             // (this call's count of the registration's iterations: tdlo_mstep_chain.hip)
            const hipError_t me = launch_estep_only(c->fd, c->fh.data(), 1, 5, s);     // M-step with the exchange of the sums inside
            mstep_parity_hint(-1);
            HIPCHK(c, me);
        } else {
            int e;
            if (visb) {
                HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 1, s));
                HIPCHK(c, launch_split_dmin_xch(c->fd, c->fh.data(), b_dmin, 0, s));
                if ((e = nccl(R->AllReduce(b_dmin, b_dmin, (size_t)M, kNcclFloat64, kNcclMin, nccl_comm, s), "ncclAllReduce(dmin)"))) return e;
                HIPCHK(c, launch_split_dmin_xch(c->fd, c->fh.data(), b_dmin, 1, s));
            }
            HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 0, s));
            HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 3, s));                // the shard's accumulators -> b_sums
            if ((e = nccl(R->AllReduce(b_sums, b_sums, 4 * (size_t)M + 2, kNcclFloat64, kNcclSum, nccl_comm, s), "ncclAllReduce(sums)"))) return e;
            HIPCHK(c, launch_estep_only(c->fd, c->fh.data(), 1, 4, s));
        }
        return 0;
    };
    IterState is{};
    int common_status = 0;              // RCCL form: the MIN over the ranks of their status
    for (int it = 1; it <= p->max_iter; ++it) {
        if ((rc = iteration())) return rc;
        // the stopping rule lives on the device (the same flag on every rank: they solve the same system); it is read after
        // iterations 1, 2, 4, 8, 12, ... -- a tracker in steady state converges within a couple of iterations.  With a communicator the
        // decision is taken TOGETHER (MIN all-reduce of [done without error, status]): a rank that stopped on an error of its own -- a
        // shard whose sums leave the fixed point's range -- must not leave its peers inside the next all-reduce
        const bool poll = p->tol > 0.0 && it < p->max_iter && (it == 1 || it == 2 || it == 4 || (it >= 8 && it % 4 == 0));
        if (poll && oneshot) {
            HIPCHK(c, hipMemcpyAsync(c->pin, f.st, sizeof(IterState), hipMemcpyDeviceToHost, s));
            HIPCHK(c, wait_stream(s));
            std::memcpy(&is, c->pin, sizeof is);
            if (is.done) break;
        } else if (poll) {
            HIPCHK(c, launch_split_poll_pack(c->fd, b_init, s));
            if ((rc = nccl(R->AllReduce(b_init, b_init, 2, kNcclFloat64, kNcclMin, nccl_comm, s), "ncclAllReduce(poll)"))) return rc;
            HIPCHK(c, hipMemcpyAsync(c->pin, b_init, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(c, wait_stream(s));
            if (c->pin[0] != 0.0 || c->pin[1] < 0.0) { common_status = (int)c->pin[1]; break; }
        }
    }
    if (!oneshot) {                     // every rank leaves with the same verdict
        HIPCHK(c, launch_split_poll_pack(c->fd, b_init, s));
        if ((rc = nccl(R->AllReduce(b_init, b_init, 2, kNcclFloat64, kNcclMin, nccl_comm, s), "ncclAllReduce(status)"))) return rc;
    }
    if (timing) HIPCHK(c, hipEventRecord(c->ev[2], s));
    HIPCHK(c, hipMemcpyAsync(c->pin, c->slots[0].nodeblk + nc.Yout, nc.readback * sizeof(double), hipMemcpyDeviceToHost, s));
    if (timing) HIPCHK(c, hipEventRecord(c->ev[3], s));
    if (!oneshot) HIPCHK(c, hipMemcpyAsync(c->pin + nc.readback, b_init, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(c, wait_stream(s));
    std::memcpy(&is, c->pin + (nc.st - nc.Yout), sizeof is);
    if (!oneshot) { common_status = (int)c->pin[nc.readback + 1]; if (common_status < 0 && is.status == 0) is.status = common_status; }
    c->last_F = 1;
    // The banded L D L^T gave up (non-positive pivot, non-finite sigma2): every rank solves the same system from the same sums, so every rank
    // is here with TDLO_E_NUMERIC (RCCL form: the common status; one-shot form: the same pivots, and a rank whose own shard failed has told
    // its peers, kXchErrMark) and repeats the call on the dense pivoted kernels, like run_frames -- Y and sigma2 are untouched so far.  The
    // one-shot exchange lives in one-workgroup kernels only: the dense k_mstep_fast serves up to 64 nodes, longer chains keep the error.
    if (is.status == TDLO_E_NUMERIC && p->include_lle && f.lle_band && !c->lle_dense_once && (!oneshot || M <= 64)) {
        c->lle_dense_once = true;
        ++c->band_retries;
        const int rr = tdlo_split_run(c, nccl_comm, Y, M, sigma2, p, priors, K, vis, n_vis, H_override, stats);
        c->lle_dense_once = false;
        if (stats) stats->band_retry = 1;
        return rr;
    }
    // fp64 mode: a share refused under the limits that follow sigma (IterState::sh_boost) would have passed the coarse ones.  As in run_frames, the
    // status does not say which check failed, so EVERY fp64 TDLO_E_NUMERIC repeats the call ONCE with the coarse limits (Y and sigma2 are untouched
    // so far; a failure of another kind -- non-finite sigma2, a singular system -- fails again and costs a second run).  The status is common to the
    // ranks (RCCL form: the MIN all-reduce above; one-shot form: a rank whose own shard failed has told its peers, kXchErrMark), so every rank
    // repeats or none does.  tdlo_debug_route_count 10 counts the repeats.
    if (p->precision == TDLO_PREC_F64 && !c->boost_off_once && p->max_iter > 0 && is.status == TDLO_E_NUMERIC) {
        c->boost_off_once = true;
        ++c->boost_retries;
        const int rr = tdlo_split_run(c, nccl_comm, Y, M, sigma2, p, priors, K, vis, n_vis, H_override, stats);
        c->boost_off_once = false;
        return rr;
    }
    if ((is.status == 0 || is.status == TDLO_E_NUMERIC) && is.it > 0) { std::memcpy(Y, c->pin, sizeof(double) * 3 * M); }
    if (is.status == 0 || is.status == TDLO_E_NUMERIC) *sigma2 = is.sigma2;
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        fill_stats(stats, is);
        if (p->max_iter == 0) stats->converged = 1;
        if (timing) { hipEventElapsedTime(&stats->loop_ms, c->ev[1], c->ev[2]); hipEventElapsedTime(&stats->total_ms, c->ev[0], c->ev[3]); }
        stats->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
    }
    if (is.status == TDLO_E_EMPTY) return fail(c, is.status, "every point of every shard was pruned (no point within 0.1 m of a node, trackdlo.cpp:190)");
    if (is.status == TDLO_E_NUMERIC) return fail(c, is.status, "non-finite or non-positive sigma2, or singular M-step system");
    if (is.status == TDLO_E_EXCHANGE) return fail(c, is.status, "a peer's contribution to the one-shot exchange did not arrive within its time limit");
    return is.status;
}

// ---- plain GMM-EM `reg` ---------------------------------------------------------------------------
// The `reg` workspace holds at least `doubles` (a context's one device scratch for reg and sort_pts: grown, never shrunk)
static int ensure_reg_ws(tdlo_ctx *c, size_t doubles) {
    if (doubles <= c->reg_ws_cap) return TDLO_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->reg_ws) hipFree(c->reg_ws);
    c->reg_ws = nullptr; c->reg_ws_cap = 0;
    HIPCHK(c, hipMalloc((void **)&c->reg_ws, doubles * sizeof(double)));
    c->reg_ws_cap = doubles;
    return TDLO_OK;
}

// reg's whole loop on the cloud resident in the slot, enqueued: state and centroids are left at reg_ws (state 8 | Y 3 M); `extra` more doubles of
// the workspace behind reg's own are handed out at *extra_dev (8-byte aligned), and the pinned staging holds 8 + 3 M + extra doubles
static int reg_enqueue(tdlo_ctx *c, Slot &s, int M, double mu, int max_iter, size_t extra, double **extra_dev) {
    const int n = s.N0;
    const int nblk = std::max(1, std::min((n + 255) / 256, 256));
    const size_t need = reg_ws_doubles(M, nblk);
    int rc;
    if ((rc = ensure_reg_ws(c, need + extra)) || (rc = ensure_pin(c, 8 + 3 * (size_t)M + extra))) return rc;
    double *h = c->pin;
    for (int i = 0; i < 8; ++i) h[i] = 0.0;
    for (int i = 0; i < M; ++i) {                                         // utils.cpp:24-29
        h[8 + i] = 0.0;
        h[8 + M + i] = 0.1 / static_cast<double>(M) * static_cast<double>(i);
        h[8 + 2 * M + i] = 0.0;
    }
    HIPCHK(c, hipMemcpyAsync(c->reg_ws, h, sizeof(double) * (8 + 3 * (size_t)M), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_reg(s.Xraw, n, M, mu, max_iter, nblk, c->reg_ws, c->stream));
    if (extra_dev) *extra_dev = c->reg_ws + need;
    return TDLO_OK;
}

int tdlo_reg(tdlo_ctx *c, int slot, const double *pts, int N, double *Y, double *sigma2, int M, double mu, int max_iter) {
    if (!c) return TDLO_E_INVALID;
    if (slot < 0 || slot >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
    if (!Y || !sigma2 || M < 1 || max_iter < 0 || !(mu >= 0 && mu < 1)) return fail(c, TDLO_E_INVALID, "bad reg arguments");
    if (M > reg_max_nodes()) return fail(c, TDLO_E_INVALID, "reg: more than " + std::to_string(reg_max_nodes()) + " centroids do not fit the E-step's per-wave accumulators in 160 KB of LDS");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = TDLO_OK;
    if (pts) rc = tdlo_set_cloud(c, slot, pts, N);
    else if (c->slots[slot].N0 <= 0) rc = fail(c, TDLO_E_INVALID, "pts is NULL and no cloud is resident in the slot");
    if (rc) return rc;
    if ((rc = reg_enqueue(c, c->slots[slot], M, mu, max_iter, 0, nullptr))) return rc;
    double *h = c->pin;
    HIPCHK(c, hipMemcpyAsync(h, c->reg_ws, sizeof(double) * (8 + 3 * (size_t)M), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *sigma2 = h[0];
    std::memcpy(Y, h + 8, sizeof(double) * 3 * (size_t)M);
    return TDLO_OK;
}

// ---- `sort_pts`: chain order and chain coordinate (csrc/tdlo_init.hip) --------------------------------------------------------------
static const char *sort_pts_reason(int status) {
    return status == 1 ? "sort_pts: a node has a non-finite coordinate"
         : status == 2 ? "sort_pts: two nodes coincide (the reference finds rows of its list by value, utils.cpp:146-150)"
                       : "sort_pts: a round found no edge (every remaining squared distance is zero or infinite)";
}

int tdlo_sort_pts_host(const double *Y, int M, double *Y_sorted, int *perm, double *coord) {
    if (!Y || M < 2 || M > kMaxNodes) return TDLO_E_INVALID;
    return sort_pts_host(Y, M, Y_sorted, perm, coord) ? TDLO_E_NUMERIC : TDLO_OK;
}

int tdlo_sort_pts(tdlo_ctx *c, const double *Y, int M, double *Y_sorted, int *perm, double *coord) {
    if (!c) return TDLO_E_INVALID;
    if (!Y || M < 2 || M > kMaxNodes) return fail(c, TDLO_E_INVALID, "sort_pts: 2 .. " + std::to_string(kMaxNodes) + " nodes");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nin = 3 * (size_t)M + 1, nout = sort_pts_out_doubles(M);      // (+ 1: the output block stays 16-byte aligned)
    int rc;
    if ((rc = ensure_reg_ws(c, nin + nout)) || (rc = ensure_pin(c, nin + nout))) return rc;
    double *h = c->pin, *ho = h + nin;
    std::memcpy(h, Y, sizeof(double) * 3 * (size_t)M);
    HIPCHK(c, hipMemcpyAsync(c->reg_ws, h, sizeof(double) * 3 * (size_t)M, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_sort_pts(c->reg_ws, nullptr, M, c->reg_ws + nin, c->stream));
    HIPCHK(c, hipMemcpyAsync(ho, c->reg_ws + nin, sizeof(double) * nout, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ++c->init_route[0];
    if (ho[1] != 0.0) return fail(c, TDLO_E_NUMERIC, sort_pts_reason((int)ho[1]));
    if (Y_sorted) std::memcpy(Y_sorted, ho + 2, sizeof(double) * 3 * (size_t)M);
    if (coord) std::memcpy(coord, ho + 2 + 3 * (size_t)M, sizeof(double) * M);
    if (perm) std::memcpy(perm, ho + 2 + 4 * (size_t)M, sizeof(int) * M);
    return TDLO_OK;
}

// ---- reg and sort_pts for F frames in one call (csrc/tdlo_reg_batch.hip, k_sort_pts_batch; the layout: csrc/tdlo_reg_plan.h) ---------------------
// From this many frames on tdlo_reg_batch, tdlo_sort_pts_batch and tdlo_tracker_initialize_from_cloud_batch let the frames share the launches; below it
// they loop over the single calls.  By the rule set beforehand -- the smallest F from which on the batch's median lies below the single calls' by more than
// both spreads, at N = 5 000 and N = 500 -- measured (profiles/init_batch_ab.txt): 1.  Two trackers start in 5.69 against 11.61 ms, 32 in 11.79 against
// 186.0 ms, and one frame through the batch launches is level with the single call (5.72 against 5.81 ms), so every batch call takes them.
// TDLO_INIT_BATCH_MIN=n, read when the context is made, overrides: below n frames the call loops over the single calls (the comparator).
constexpr int kInitBatchMin = 1;
static int init_batch_min(const tdlo_ctx *c) { return c->init_batch_min ? c->init_batch_min : kInitBatchMin; }

static_assert(sizeof(RegBatchFrame) == 4 * sizeof(double), "the frame table is carved out of the workspace in doubles");

// what the slots of a batch must be (in range, distinct, a cloud resident in each): the reason they are not, or nullptr
static const char *batch_slots_refusal(const tdlo_ctx *c, const int *slots, int F) {
    for (int f = 0; f < F; ++f) {
        if (slots[f] < 0 || slots[f] >= (int)c->slots.size()) return "a slot is out of range";
        for (int g = 0; g < f; ++g) if (slots[g] == slots[f]) return "a slot is named twice";
        if (c->slots[slots[f]].N0 <= 0) return "no cloud is resident in a slot";
    }
    return nullptr;
}

// Where a batched start keeps things.  Device (reg_ws): [frame table 4 F | plan: F states | partials | F output blocks]; pinned staging: [frame table |
// F start states | read-back: F states or F output blocks]
struct RegBatchRun {
    long long S = 0, O = 0;              // strides of the state and of the output blocks
    double *states_dev = nullptr, *outs_dev = nullptr;
    double *readback = nullptr;          // pinned
};

// reg's whole loop for the clouds resident in F slots, enqueued: one upload (table and start states), then the 2 + 2 max_iter launches.  The arguments
// have been checked (batch_slots_refusal, M, mu, max_iter).
static int reg_batch_enqueue(tdlo_ctx *c, const int *slots, int F, int M, double mu, int max_iter, RegBatchRun &run) {
    std::vector<int> N(F), nblk(F);
    std::vector<long long> state_off(F), part_off(F), out_off(F);
    long long total = 0;
    for (int f = 0; f < F; ++f) N[f] = c->slots[slots[f]].N0;
    if (reg_batch_plan(N.data(), F, M, nblk.data(), state_off.data(), part_off.data(), out_off.data(), &total)) return fail(c, TDLO_E_INVALID, "reg batch: no plan");
    const size_t T = 4 * (size_t)F;
    run.S = reg_plan_state_stride(M); run.O = reg_plan_out_stride(M);
    const size_t up = T + (size_t)run.S * F;
    int rc;
    if ((rc = ensure_reg_ws(c, T + (size_t)total)) || (rc = ensure_pin(c, up + (size_t)std::max(run.S, run.O) * F))) return rc;
    double *base = c->reg_ws + T;
    run.states_dev = base; run.outs_dev = base + out_off[0]; run.readback = c->pin + up;
    RegBatchFrame *tab = reinterpret_cast<RegBatchFrame *>(c->pin);
    int max_nblk = 1;
    for (int f = 0; f < F; ++f) {
        tab[f] = RegBatchFrame{c->slots[slots[f]].Xraw, base + state_off[f], base + part_off[f], N[f], nblk[f]};
        max_nblk = std::max(max_nblk, nblk[f]);
        double *h = c->pin + T + (size_t)run.S * f;
        for (long long i = 0; i < run.S; ++i) h[i] = 0.0;
        for (int i = 0; i < M; ++i) h[8 + M + i] = 0.1 / static_cast<double>(M) * static_cast<double>(i);      // utils.cpp:24-29, as reg_enqueue
    }
    HIPCHK(c, hipMemcpyAsync(c->reg_ws, c->pin, sizeof(double) * up, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_reg_batch(reinterpret_cast<const RegBatchFrame *>(c->reg_ws), F, max_nblk, M, mu, max_iter, c->stream));
    return TDLO_OK;
}

int tdlo_reg_batch(tdlo_ctx *c, const int *slots, int F, double *Y, double *sigma2, int M, double mu, int max_iter) {
    if (!c) return TDLO_E_INVALID;
    if (!slots || F < 1 || !Y || !sigma2 || M < 1 || max_iter < 0 || !(mu >= 0 && mu < 1)) return fail(c, TDLO_E_INVALID, "reg batch: bad reg arguments");
    if (M > reg_max_nodes()) return fail(c, TDLO_E_INVALID, "reg batch: more than " + std::to_string(reg_max_nodes()) + " centroids do not fit the E-step's per-wave accumulators in 160 KB of LDS");
    if (const char *why = batch_slots_refusal(c, slots, F)) return fail(c, TDLO_E_INVALID, std::string("reg batch: ") + why);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = flush_pending_cloud(c))) return rc;
    const size_t YM = 3 * (size_t)M;
    if (F < init_batch_min(c)) {
        for (int f = 0; f < F; ++f) {
            if ((rc = tdlo_reg(c, slots[f], nullptr, 0, Y + YM * f, sigma2 + f, M, mu, max_iter))) return rc;
            ++c->ibat_route[1];
        }
        return TDLO_OK;
    }
    RegBatchRun run;
    if ((rc = reg_batch_enqueue(c, slots, F, M, mu, max_iter, run))) return rc;
    HIPCHK(c, hipMemcpyAsync(run.readback, run.states_dev, sizeof(double) * (size_t)run.S * F, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ibat_route[0] += F;
    for (int f = 0; f < F; ++f) {
        const double *h = run.readback + (size_t)run.S * f;
        sigma2[f] = h[0];
        std::memcpy(Y + YM * f, h + 8, sizeof(double) * YM);
    }
    return TDLO_OK;
}

int tdlo_sort_pts_batch(tdlo_ctx *c, const double *Y, int F, int M, double *Y_sorted, int *perm, double *coord, int *rc_each) {
    if (!c) return TDLO_E_INVALID;
    if (!Y || F < 1) return fail(c, TDLO_E_INVALID, "sort_pts batch: no node sets");
    if (M < 2 || M > kMaxNodes) return fail(c, TDLO_E_INVALID, "sort_pts batch: 2 .. " + std::to_string(kMaxNodes) + " nodes");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t YM = 3 * (size_t)M;
    std::vector<int> rcs(F, 0);
    std::string why;
    int first = -1;
    auto failed = [&](int f, int code, const std::string &text) {
        rcs[f] = code;
        if (first < 0) { first = f; why = text; }
    };
    int rc;
    if (F < init_batch_min(c)) {
        for (int f = 0; f < F; ++f) {
            rc = tdlo_sort_pts(c, Y + YM * f, M, Y_sorted ? Y_sorted + YM * f : nullptr, perm ? perm + (size_t)M * f : nullptr, coord ? coord + (size_t)M * f : nullptr);
            if (rc && rc != TDLO_E_NUMERIC) return rc;
            if (rc) failed(f, rc, c->err);
            ++c->ibat_route[1];
        }
    } else {
        const size_t I = YM + (YM & 1), O = (size_t)reg_plan_out_stride(M);       // every node set and every output block on 16 bytes
        if ((rc = ensure_reg_ws(c, (I + O) * F)) || (rc = ensure_pin(c, (I + O) * F))) return rc;
        double *h = c->pin, *ho = h + I * F, *out_dev = c->reg_ws + I * F;
        for (int f = 0; f < F; ++f) std::memcpy(h + I * f, Y + YM * f, sizeof(double) * YM);
        HIPCHK(c, hipMemcpyAsync(c->reg_ws, h, sizeof(double) * I * F, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_sort_pts_batch(c->reg_ws, (long long)I, false, F, M, out_dev, (long long)O, c->stream));
        HIPCHK(c, hipMemcpyAsync(ho, out_dev, sizeof(double) * O * F, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->ibat_route[0] += F;
        for (int f = 0; f < F; ++f) {
            const double *o = ho + O * f;
            if (o[1] != 0.0) { failed(f, TDLO_E_NUMERIC, sort_pts_reason((int)o[1])); continue; }
            if (Y_sorted) std::memcpy(Y_sorted + YM * f, o + 2, sizeof(double) * YM);
            if (coord) std::memcpy(coord + (size_t)M * f, o + 2 + YM, sizeof(double) * M);
            if (perm) std::memcpy(perm + (size_t)M * f, o + 2 + 4 * (size_t)M, sizeof(int) * M);
        }
    }
    if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
    if (first >= 0) return fail(c, rcs[first], "sort_pts batch: frame " + std::to_string(first) + ": " + why);
    return TDLO_OK;
}

int tdlo_debug_reg_batch_plan(const int *N, int F, int M, int *nblk, long long *state_off, long long *part_off, long long *out_off, long long *total) {
    return reg_batch_plan(N, F, M, nblk, state_off, part_off, out_off, total) ? TDLO_E_INVALID : TDLO_OK;
}

// Waits for the one-launch kernel's word in pinned host memory (epoch << 32 | status); like mbox_wait, the stream is looked at every 0.5 ms so that
// a faulting kernel cannot hang the caller.  Returns the status (1, 2, 3), 0 when the stream drained without the word, or a negative code.
static int cloud_wait(tdlo_ctx *c, hipStream_t st, unsigned epoch) {
    auto t_chk = std::chrono::steady_clock::now();
    for (unsigned spins = 1;; ++spins) {
        const unsigned long long v = __atomic_load_n(c->cloud_res, __ATOMIC_ACQUIRE);
        if ((unsigned)(v >> 32) == epoch) return (int)(unsigned)v;
        if ((spins & 255u) == 0) {
            const auto now = std::chrono::steady_clock::now();
            if (std::chrono::duration<double, std::micro>(now - t_chk).count() > 500.0) {
                t_chk = now;
                const hipError_t e = hipStreamQuery(st);
                if (e == hipSuccess) {
                    const unsigned long long v2 = __atomic_load_n(c->cloud_res, __ATOMIC_ACQUIRE);
                    return (unsigned)(v2 >> 32) == epoch ? (int)(unsigned)v2 : 0;
                }
                if (e != hipErrorNotReady) return fail(c, TDLO_E_HIP, std::string("stream: ") + hipGetErrorString(e));
            }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
}

static size_t img_depth_bytes(size_t P) { return (P * 2 + 255) & ~(size_t)255; }
static size_t img_mask_bytes(size_t P) { return (P + 255) & ~(size_t)255; }

int tdlo_image_buffers(tdlo_ctx *c, int rows, int cols, unsigned short **depth, unsigned char **mask) {
    if (!c) return TDLO_E_INVALID;
    if (rows <= 0 || cols <= 0 || (long long)rows * cols > (1ll << 26) || !depth || !mask) return fail(c, TDLO_E_INVALID, "bad image");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t P = (size_t)rows * cols, need = img_depth_bytes(P) + img_mask_bytes(P);
    if (need > c->img_pin_cap) {
        HIPCHK(c, drain_for_realloc(c));
        if (c->img_pin) hipHostFree(c->img_pin);
        c->img_pin = nullptr; c->img_pin_cap = 0;
        HIPCHK(c, hipHostMalloc((void **)&c->img_pin, need, hipHostMallocDefault));
        std::memset(c->img_pin, 0, need);
        c->img_pin_cap = need;
    }
    c->img_pin_rows = rows; c->img_pin_cols = cols;
    *depth = (unsigned short *)c->img_pin;
    *mask = (unsigned char *)(c->img_pin + img_depth_bytes(P));
    return TDLO_OK;
}

// ---- colour segmentation in front of depth -> cloud (trackdlo_node.cpp:84-119, :158-180) -------------------------------
static size_t img_colour_bytes(size_t P) { return (3 * P + 16 + 255) & ~(size_t)255; }      // (the last thread's 12-byte load ends up to 9 bytes beyond the image)
static size_t img_occ_bytes(size_t P) { return (P + 16 + 255) & ~(size_t)255; }

struct ColourIn { const unsigned char *colour; const tdlo_colour_params *params; const unsigned char *occluder; };

// tdlo_colour_params as the kernels take it: bounds clamped to 0 .. 255 and packed H | S << 8 | V << 16, upper - lower per channel beside them; a range
// whose lower bound lies above its upper bound on a channel passes nothing and is left out
// (the rule itself is colour_ranges_pack, tdlo_rig_host.cpp: HIP-free, so that the host half of a rig packs by the same statement)
static bool colour_pack(const tdlo_colour_params *p, CloudColour &cc) {
    cc = CloudColour{};
    return colour_ranges_pack(p, cc.lo, cc.span, &cc.n, &cc.rgb);
}

int tdlo_colour_buffers(tdlo_ctx *c, int rows, int cols, unsigned char **colour, unsigned char **occluder) {
    if (!c) return TDLO_E_INVALID;
    if (rows <= 0 || cols <= 0 || (long long)rows * cols > (1ll << 26) || !colour || !occluder) return fail(c, TDLO_E_INVALID, "bad image");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t P = (size_t)rows * cols, need = img_colour_bytes(P) + img_occ_bytes(P);
    if (need > c->col_pin_cap) {
        HIPCHK(c, drain_for_realloc(c));
        if (c->col_pin) hipHostFree(c->col_pin);
        if (c->last_colour == (const unsigned char *)c->col_pin) c->last_colour = c->last_occluder = nullptr;      // (a render call has nothing to draw over until the next colour call)
        c->col_pin = nullptr; c->col_pin_cap = 0;
        HIPCHK(c, hipHostMalloc((void **)&c->col_pin, need, hipHostMallocDefault));
        std::memset(c->col_pin, 0, need);
        c->col_pin_cap = need;
    }
    c->col_pin_rows = rows; c->col_pin_cols = cols;
    *colour = (unsigned char *)c->col_pin;
    *occluder = (unsigned char *)(c->col_pin + img_colour_bytes(P));
    return TDLO_OK;
}

// where the kernels read the frame's colour and occluder images: the context's pinned buffers when the caller passes exactly those (tdlo_colour_buffers),
// else device copies made here; *d_hsv (optional): room for the HSV image behind them
static int colour_stage(tdlo_ctx *c, const ColourIn &ci, int rows, int cols, CloudColour &cc, unsigned char **d_hsv) {
    const size_t P = (size_t)rows * cols;
    const size_t need = img_colour_bytes(P) + img_occ_bytes(P) + (d_hsv ? img_colour_bytes(P) : 0);
    const bool in_place = c->col_pin != nullptr && (const char *)ci.colour == c->col_pin && c->col_pin_rows == rows && c->col_pin_cols == cols &&
                          (!ci.occluder || (const char *)ci.occluder == c->col_pin + img_colour_bytes(P));
    // a view call's import has written the images into the device buffers already (stage_frame_view sized them): nothing to copy
    const bool on_dev = c->col_dev != nullptr && (const void *)ci.colour == c->col_dev && !d_hsv && need <= c->col_dev_cap &&
                        (!ci.occluder || (const char *)ci.occluder == (const char *)c->col_dev + img_colour_bytes(P));
    c->last_colour = c->last_occluder = nullptr;
    if ((!in_place || d_hsv) && need > c->col_dev_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->col_dev) hipFree(c->col_dev);
        c->col_dev = nullptr; c->col_dev_cap = 0;
        HIPCHK(c, hipMalloc(&c->col_dev, need));
        c->col_dev_cap = need;
    }
    char *base = (char *)c->col_dev;
    if (in_place || on_dev) { cc.colour = ci.colour; cc.occluder = ci.occluder; }
    else {
        cc.colour = (const unsigned char *)base;
        cc.occluder = ci.occluder ? (const unsigned char *)(base + img_colour_bytes(P)) : nullptr;
        HIPCHK(c, hipMemcpyAsync(base, ci.colour, 3 * P, hipMemcpyHostToDevice, c->stream));
        if (ci.occluder) HIPCHK(c, hipMemcpyAsync(base + img_colour_bytes(P), ci.occluder, P, hipMemcpyHostToDevice, c->stream));
    }
    if (d_hsv) *d_hsv = (unsigned char *)(base + img_colour_bytes(P) + img_occ_bytes(P));
    c->last_colour = cc.colour; c->last_occluder = cc.occluder; c->last_col_rows = rows; c->last_col_cols = cols;      // (tdlo_render_result with colour == NULL)
    return TDLO_OK;
}

static int ensure_cloud_ws(tdlo_ctx *c, int P);

// The segmentation on its own (k_colour_mask): the mask goes into the context's device mask buffer (where the multi-launch depth -> cloud form reads it) and,
// when asked for, to the host together with the HSV image
int tdlo_colour_mask(tdlo_ctx *c, const unsigned char *colour, int rows, int cols, const tdlo_colour_params *params, const unsigned char *occluder,
                     unsigned char *mask_out, unsigned char *hsv_out) {
    if (!c) return TDLO_E_INVALID;
    CloudColour cc;
    if (!colour_pack(params, cc)) return fail(c, TDLO_E_INVALID, "tdlo_colour_params: 1 .. 4 ranges");
    if (!colour || rows <= 0 || cols <= 0 || (long long)rows * cols > (1ll << 26)) return fail(c, TDLO_E_INVALID, "bad image");
    HIPCHK(c, hipSetDevice(c->device));
    const int P = rows * cols;
    int rc = ensure_cloud_ws(c, P);
    if (rc) return rc;
    unsigned char *d_hsv = nullptr;
    const ColourIn ci{colour, params, occluder};
    if ((rc = colour_stage(c, ci, rows, cols, cc, hsv_out ? &d_hsv : nullptr))) return rc;
    unsigned char *d_mask = (unsigned char *)c->cloud_ws + img_depth_bytes(P);
    HIPCHK(c, launch_colour_mask(cc, P, d_mask, d_hsv, c->stream));
    if (mask_out) HIPCHK(c, hipMemcpyAsync(mask_out, d_mask, (size_t)P, hipMemcpyDeviceToHost, c->stream));
    if (hsv_out) HIPCHK(c, hipMemcpyAsync(hsv_out, d_hsv, 3 * (size_t)P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TDLO_OK;
}

// ---- the tracking-result image (trackdlo_node.cpp:377-452): blend, edges and nodes in one launch (tdlo_render.hip) ------------------------------------
static constexpr size_t kRenderPrimBytes = (size_t)3 * (kMaxNodes - 1) * 8 * sizeof(int);      // the table of the longest chain; the two corner words behind it

void tdlo_default_render_params(tdlo_render_params *p) {
    if (!p) return;
    const tdlo_render_params d = {5, 7, {0, 150, 255}, {0, 0, 255}, {0, 255, 0}, {0, 0, 255}};      // :409-440, bytes in the image's order (the node's bgr8)
    *p = d;
}

int tdlo_render_primitives(const double *Y, int M, const double proj[12], const int *vis, int n_vis, const tdlo_render_params *p, int *prims, int *n_prims) {
    tdlo_render_params d;
    tdlo_default_render_params(&d);
    if (!p) p = &d;
    if (!prims || !n_prims) return TDLO_E_INVALID;
    if (render_primitives(Y, M, proj, vis, n_vis, p->line_width, p->node_radius, p->node_visible, p->node_hidden, p->edge_visible, p->edge_hidden, prims)) return TDLO_E_INVALID;
    *n_prims = 3 * (M - 1);
    return TDLO_OK;
}

int tdlo_result_image_buffer(tdlo_ctx *c, int rows, int cols, unsigned char **image) {
    if (!c) return TDLO_E_INVALID;
    if (rows <= 0 || cols <= 0 || rows > 8192 || cols > 8192 || !image) return fail(c, TDLO_E_INVALID, "bad image");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t need = img_colour_bytes((size_t)rows * cols);
    if (need > c->res_pin_cap) {
        HIPCHK(c, drain_for_realloc(c));
        if (c->res_pin) hipHostFree(c->res_pin);
        c->res_pin = nullptr; c->res_pin_cap = 0;
        HIPCHK(c, hipHostMalloc((void **)&c->res_pin, need, hipHostMallocDefault));
        std::memset(c->res_pin, 0, need);
        c->res_pin_cap = need;
    }
    c->res_pin_rows = rows; c->res_pin_cols = cols;
    *image = (unsigned char *)c->res_pin;
    return TDLO_OK;
}

int tdlo_last_colour_shape(tdlo_ctx *c, int *rows, int *cols) {
    if (!c) return TDLO_E_INVALID;
    if (!rows || !cols) return fail(c, TDLO_E_INVALID, "tdlo_last_colour_shape: rows and cols");
    if (!c->last_colour) return fail(c, TDLO_E_INVALID, "no colour call of this context yet");
    *rows = c->last_col_rows; *cols = c->last_col_cols;
    return TDLO_OK;
}

int tdlo_render_result(tdlo_ctx *c, const unsigned char *colour, const unsigned char *occluder, int rows, int cols, const double *Y, int M, const double proj[12],
                       const int *vis, int n_vis, const tdlo_render_params *p, unsigned char *image_out, int corners[4]) {
    if (!c) return TDLO_E_INVALID;
    // everything that can be refused is refused before the first byte of image_out is written
    if (rows <= 0 || cols <= 0 || rows > 8192 || cols > 8192 || !image_out) return fail(c, TDLO_E_INVALID, "tdlo_render_result: images of 1 .. 8192 rows and columns");
    if (!Y || !proj || M < 1 || M > kMaxNodes) return fail(c, TDLO_E_INVALID, "tdlo_render_result: 1 .. 1024 nodes and a projection matrix");
    if (!colour && !(c->last_colour && c->last_col_rows == rows && c->last_col_cols == cols))
        return fail(c, TDLO_E_INVALID, "tdlo_render_result: colour == NULL needs a colour call of this context on an image of the same shape before it");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->rnd_pin) {
        HIPCHK(c, hipHostMalloc((void **)&c->rnd_pin, kRenderPrimBytes + 16, hipHostMallocDefault));
        const hipError_t e = hipMalloc((void **)&c->rnd_dev, kRenderPrimBytes + 16);
        if (e != hipSuccess) { hipHostFree(c->rnd_pin); c->rnd_pin = nullptr; c->rnd_dev = nullptr; return fail(c, TDLO_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    }
    int n_prims = 0;
    if (tdlo_render_primitives(Y, M, proj, vis, n_vis, p, (int *)c->rnd_pin, &n_prims))        // (the staging table is free: every call returns with the stream drained)
        return fail(c, TDLO_E_INVALID, "tdlo_render_result: a node that cannot be drawn (w <= 0, a non-finite pixel, a pixel beyond +-8192), vis out of range, or a "
                                       "line width / node radius outside 1 .. 255");
    // where the image goes: the pinned result buffer and device memory are written by the kernel itself; anything else (and everything under
    // TDLO_RENDER_INPLACE=0) receives a copy of the device image
    const size_t P = (size_t)rows * cols;
    bool out_device = false;
    const bool out_pinned = c->res_pin != nullptr && (char *)image_out == c->res_pin && c->res_pin_rows == rows && c->res_pin_cols == cols;
    if (!out_pinned) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, image_out) != hipSuccess) (void)hipGetLastError();      // (a pointer the runtime does not know: host memory)
        else if (at.type == hipMemoryTypeDevice) {
            if (at.device != c->device) return fail(c, TDLO_E_INVALID, "tdlo_render_result: image_out is device memory of another GPU");
            out_device = true;
        }
    }
    const bool direct = c->render_inplace && (out_pinned || (out_device && (uintptr_t)image_out % 4 == 0));
    if (!direct && img_colour_bytes(P) > c->res_dev_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->res_dev) hipFree(c->res_dev);
        c->res_dev = nullptr; c->res_dev_cap = 0;
        HIPCHK(c, hipMalloc(&c->res_dev, img_colour_bytes(P)));
        c->res_dev_cap = img_colour_bytes(P);
    }
    const unsigned char *d_colour = c->last_colour, *d_occ = c->last_occluder;
    if (colour) {
        CloudColour cc{};
        const ColourIn ci{colour, nullptr, occluder};
        if (int rc = colour_stage(c, ci, rows, cols, cc, nullptr)) return rc;
        d_colour = cc.colour; d_occ = cc.occluder;
    }
    hipStream_t st = c->stream;
    unsigned *d_corner = (unsigned *)(c->rnd_dev + kRenderPrimBytes), *h_corner = (unsigned *)(c->rnd_pin + kRenderPrimBytes);
    if (n_prims) HIPCHK(c, hipMemcpyAsync(c->rnd_dev, c->rnd_pin, (size_t)n_prims * 8 * sizeof(int), hipMemcpyHostToDevice, st));
    if (d_occ && corners) HIPCHK(c, hipMemsetAsync(d_corner, 0xff, 8, st));                        // {0xffffffff, -1}: no zero byte seen
    unsigned char *d_out = direct ? image_out : (unsigned char *)c->res_dev;
    HIPCHK(c, launch_render(d_colour, d_occ, d_out, (const int *)c->rnd_dev, n_prims, (int)P, cols, (d_occ && corners) ? d_corner : nullptr, st));
    if (!direct) HIPCHK(c, hipMemcpyAsync(image_out, c->res_dev, 3 * P, out_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    if (d_occ && corners) HIPCHK(c, hipMemcpyAsync(h_corner, d_corner, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, wait_stream(st));
    ++c->render_route[direct ? 0 : 1];
    if (corners) {
        corners[0] = corners[1] = corners[2] = corners[3] = -1;
        if (d_occ && h_corner[0] != 0xffffffffu) {
            corners[0] = (int)(h_corner[0] / (unsigned)cols); corners[1] = (int)(h_corner[0] % (unsigned)cols);
            corners[2] = (int)(h_corner[1] / (unsigned)cols); corners[3] = (int)(h_corner[1] % (unsigned)cols);
        }
    }
    return TDLO_OK;
}

// ---- result images for many ropes: several ropes per image, K images per launch (tdlo_render_batch.hip) -------------------------------------------------
int tdlo_render_batch_table(const tdlo_render_rope *ropes, int R, int K, int *heads, int *prims, int prims_cap, int *n_prims, int *rope_first) {
    if (R < 0 || R > 1024 || K < 1 || K > 256 || (R > 0 && (!ropes || !heads)) || prims_cap < 0 || !n_prims || !rope_first) return TDLO_E_INVALID;
    tdlo_render_params d;
    tdlo_default_render_params(&d);
    std::vector<int> order, hd, pr, first;
    if (render_batch_table(ropes, R, K, d, order, hd, pr, first) >= 0) return TDLO_E_INVALID;
    if (pr.size() / 8 > (size_t)prims_cap || (!pr.empty() && !prims)) return TDLO_E_INVALID;
    std::copy(hd.begin(), hd.end(), heads);
    std::copy(pr.begin(), pr.end(), prims);
    std::copy(first.begin(), first.end(), rope_first);
    *n_prims = (int)(pr.size() / 8);
    return TDLO_OK;
}

int tdlo_render_result_batch(tdlo_ctx *c, const tdlo_render_image *images, int K, int rows, int cols, const tdlo_render_rope *ropes, int R, int *corners) {
    if (!c) return TDLO_E_INVALID;
    // everything that can be refused is refused before the first byte of any image_out is written
    if (K < 1 || K > 256 || !images) return fail(c, TDLO_E_INVALID, "tdlo_render_result_batch: 1 .. 256 images");
    if (rows <= 0 || cols <= 0 || rows > 8192 || cols > 8192) return fail(c, TDLO_E_INVALID, "tdlo_render_result_batch: images of 1 .. 8192 rows and columns");
    if (R < 0 || R > 1024 || (R > 0 && !ropes)) return fail(c, TDLO_E_INVALID, "tdlo_render_result_batch: 0 .. 1024 ropes");
    HIPCHK(c, hipSetDevice(c->device));
    tdlo_render_params dflt;
    tdlo_default_render_params(&dflt);
    std::vector<int> order, heads, prims, rope_first;
    {
        const int bad = render_batch_table(ropes, R, K, dflt, order, heads, prims, rope_first);
        if (bad >= 0)
            return fail(c, TDLO_E_INVALID, "tdlo_render_result_batch: rope " + std::to_string(bad) + ": an image outside 0 .. K - 1, not 1 .. 1024 nodes with a projection "
                                           "matrix, a node that cannot be drawn (w <= 0, a non-finite pixel, a pixel beyond +-8192), vis out of range, or a line width / "
                                           "node radius outside 1 .. 255");
    }
    const size_t P = (size_t)rows * cols, n_prims = prims.size() / 8;
    // ---- where every plane lies.  Sources: the context's pinned colour buffers and 4-byte aligned device memory are read in place, anything else is
    // staged; destinations: the pinned result buffer and 4-byte aligned device memory are written by the kernel, anything else receives a copy
    enum { kHost = 0, kDevice = 1, kOtherGpu = 2 };
    auto where = [&](const void *p) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return (int)kHost; }      // (a pointer the runtime does not know: host memory)
        if (at.type != hipMemoryTypeDevice) return (int)kHost;
        return at.device == c->device ? (int)kDevice : (int)kOtherGpu;
    };
    const bool pin_shape = c->col_pin != nullptr && c->col_pin_rows == rows && c->col_pin_cols == cols;
    struct Src { const unsigned char *p; bool occ, dev; size_t off; };
    std::vector<Src> staged;                                   // every distinct (pointer, kind) once
    struct Img { const unsigned char *colour, *occluder; long long colour_at, occ_at, out_at; bool out_dev; };      // *_at >= 0: an offset into the arena
    std::vector<Img> im(K);
    size_t stage_bytes = 0, out_bytes = 0;
    int n_direct = 0;
    auto source = [&](const unsigned char *p, bool occ, int k, const unsigned char *&in_place, long long &at) -> int {
        in_place = nullptr; at = -1;
        const bool pinned = pin_shape && (const char *)p == (occ ? c->col_pin + img_colour_bytes(P) : c->col_pin);
        int w = kHost;
        if (!pinned && (w = where(p)) == kOtherGpu)
            return fail(c, TDLO_E_INVALID, "tdlo_render_result_batch: image " + std::to_string(k) + (occ ? ": occluder" : ": colour") + " is device memory of another GPU");
        if (pinned || (w == kDevice && (uintptr_t)p % 4 == 0)) { in_place = p; return TDLO_OK; }
        size_t j = 0;
        while (j < staged.size() && !(staged[j].p == p && staged[j].occ == occ)) ++j;
        if (j == staged.size()) { staged.push_back(Src{p, occ, w == kDevice, stage_bytes}); stage_bytes += occ ? img_occ_bytes(P) : img_colour_bytes(P); }
        at = (long long)staged[j].off;
        return TDLO_OK;
    };
    for (int k = 0; k < K; ++k) {
        const tdlo_render_image &g = images[k];
        Img &m = im[k];
        m = Img{nullptr, nullptr, -1, -1, -1, false};
        if (!g.image_out) return fail(c, TDLO_E_INVALID, "tdlo_render_result_batch: image " + std::to_string(k) + " has no image_out");
        for (int j = 0; j < k; ++j)
            if (images[j].image_out == g.image_out)
                return fail(c, TDLO_E_INVALID, "tdlo_render_result_batch: images " + std::to_string(j) + " and " + std::to_string(k) + " have the same image_out");
        if (!g.colour) {
            if (!(c->last_colour && c->last_col_rows == rows && c->last_col_cols == cols))
                return fail(c, TDLO_E_INVALID, "tdlo_render_result_batch: image " + std::to_string(k) + ": colour == NULL needs a colour call of this context on an image of "
                                               "the same shape before it");
            m.colour = c->last_colour; m.occluder = c->last_occluder;
        } else {
            if (int rc = source(g.colour, false, k, m.colour, m.colour_at)) return rc;
            if (g.occluder) { if (int rc = source(g.occluder, true, k, m.occluder, m.occ_at)) return rc; }
        }
        const bool out_pinned = c->res_pin != nullptr && (char *)g.image_out == c->res_pin && c->res_pin_rows == rows && c->res_pin_cols == cols;
        if (!out_pinned) {
            const int w = where(g.image_out);
            if (w == kOtherGpu) return fail(c, TDLO_E_INVALID, "tdlo_render_result_batch: image " + std::to_string(k) + ": image_out is device memory of another GPU");
            m.out_dev = w == kDevice;
        }
        if (c->render_inplace && (out_pinned || (m.out_dev && (uintptr_t)g.image_out % 4 == 0))) ++n_direct;
        else { m.out_at = (long long)out_bytes; out_bytes += img_colour_bytes(P); }
    }
    // ---- the arena (grown on demand)
    auto r256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t tab_img = r256(sizeof(RenderBatchImage) * (size_t)K), tab_head = r256(32 * (size_t)R), tab_prim = r256(32 * n_prims);
    const size_t tab = tab_img + tab_head + tab_prim, corner_bytes = r256(8 * (size_t)K);
    const size_t dev_need = tab + corner_bytes + stage_bytes + out_bytes, pin_need = tab + corner_bytes;
    hipStream_t st = c->stream;
    if (dev_need > c->rbat_dev_cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->rbat_dev) hipFree(c->rbat_dev);
        c->rbat_dev = nullptr; c->rbat_dev_cap = 0;
        HIPCHK(c, hipMalloc((void **)&c->rbat_dev, dev_need));
        c->rbat_dev_cap = dev_need;
    }
    if (pin_need > c->rbat_pin_cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->rbat_pin) hipHostFree(c->rbat_pin);
        c->rbat_pin = nullptr; c->rbat_pin_cap = 0;
        HIPCHK(c, hipHostMalloc((void **)&c->rbat_pin, pin_need, hipHostMallocDefault));
        std::memset(c->rbat_pin, 0, pin_need);
        c->rbat_pin_cap = pin_need;
    }
    char *d_tab = c->rbat_dev, *d_corner = d_tab + tab, *d_stage = d_corner + corner_bytes, *d_out = d_stage + stage_bytes;
    char *h_tab = c->rbat_pin;                                 // (free: every call returns with the stream drained)
    const unsigned *h_corner = (const unsigned *)(c->rbat_pin + tab);
    bool any_corner = false;
    {
        RenderBatchImage *rec = (RenderBatchImage *)h_tab;
        for (int k = 0; k < K; ++k) {
            const Img &m = im[k];
            rec[k].colour = m.colour_at >= 0 ? (const unsigned char *)(d_stage + m.colour_at) : m.colour;
            rec[k].occluder = m.occ_at >= 0 ? (const unsigned char *)(d_stage + m.occ_at) : m.occluder;
            rec[k].out = m.out_at >= 0 ? (unsigned char *)(d_out + m.out_at) : images[k].image_out;
            rec[k].rope_lo = rope_first[k]; rec[k].rope_hi = rope_first[k + 1];
            rec[k].corner = (corners && rec[k].occluder) ? k : -1;
            rec[k].pad = 0;
            any_corner = any_corner || rec[k].corner >= 0;
        }
        if (R) std::memcpy(h_tab + tab_img, heads.data(), 32 * (size_t)R);
        if (n_prims) std::memcpy(h_tab + tab_img + tab_head, prims.data(), 32 * n_prims);
    }
    // ---- uploads, one launch, the copies out, one read-back, one wait
    HIPCHK(c, hipMemcpyAsync(d_tab, h_tab, tab_img + tab_head + 32 * n_prims, hipMemcpyHostToDevice, st));
    for (const Src &s : staged)
        HIPCHK(c, hipMemcpyAsync(d_stage + s.off, s.p, s.occ ? P : 3 * P, s.dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (any_corner) HIPCHK(c, hipMemsetAsync(d_corner, 0xff, 8 * (size_t)K, st));                  // {0xffffffff, -1} per image: no zero byte seen
    HIPCHK(c, launch_render_batch((const RenderBatchImage *)d_tab, K, (const int *)(d_tab + tab_img), (const int *)(d_tab + tab_img + tab_head), (int)P, cols,
                                  (unsigned *)d_corner, st));
    for (int k = 0; k < K; ++k)
        if (im[k].out_at >= 0)
            HIPCHK(c, hipMemcpyAsync(images[k].image_out, d_out + im[k].out_at, 3 * P, im[k].out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    if (any_corner) HIPCHK(c, hipMemcpyAsync((void *)h_corner, d_corner, 8 * (size_t)K, hipMemcpyDeviceToHost, st));
    HIPCHK(c, wait_stream(st));
    c->rbat_route[0] += n_direct; c->rbat_route[1] += K - n_direct;
    if (corners)
        for (int k = 0; k < K; ++k) {
            int *q = corners + 4 * (size_t)k;
            q[0] = q[1] = q[2] = q[3] = -1;
            const unsigned *h = h_corner + 2 * (size_t)k;
            if (((const RenderBatchImage *)h_tab)[k].corner >= 0 && h[0] != 0xffffffffu) {
                q[0] = (int)(h[0] / (unsigned)cols); q[1] = (int)(h[0] % (unsigned)cols);
                q[2] = (int)(h[1] / (unsigned)cols); q[3] = (int)(h[1] % (unsigned)cols);
            }
        }
    return TDLO_OK;
}

// the visibility pre-pass's device / pinned words (shared by tdlo_visibility_prepass's one-launch route and the depth -> cloud team kernel's own pre-pass)
static int ensure_vis_state(tdlo_ctx *c) {
    if (!c->vis_state) {
        HIPCHK(c, hipMalloc((void **)&c->vis_state, sizeof(unsigned long long) * (kMaxNodes + 8)));
        HIPCHK(c, hipHostMalloc((void **)&c->vis_res, sizeof(unsigned long long) * (kMaxNodes + 8), hipHostMallocDefault));
        std::memset(c->vis_res, 0, sizeof(unsigned long long) * (kMaxNodes + 8));
        c->vis_armed = false;
    }
    if (!c->vis_armed) {
        std::vector<unsigned long long> init(kMaxNodes + 8, 0x7ff0000000000000ull);
        for (int i = kMaxNodes; i < kMaxNodes + 8; ++i) init[i] = 0ull;
        HIPCHK(c, hipMemcpy(c->vis_state, init.data(), sizeof(unsigned long long) * init.size(), hipMemcpyHostToDevice));
        c->vis_armed = true;
    }
    return TDLO_OK;
}

// vis_Y != nullptr: the caller wants the frame's visibility pre-pass as well; *vis_done = true when the one-launch team kernel has left the M squared
// minima in c->vis_res[1 ..] (otherwise the caller runs tdlo_visibility_prepass on the resident cloud)
static int ensure_cloud_ws(tdlo_ctx *c, int P) {      // the device images (depth | mask) and the multi-launch form's workspace behind them
    const size_t need = img_depth_bytes(P) + img_mask_bytes(P) + cloud_ws_bytes(P);
    if (need > c->cloud_ws_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->cloud_ws) hipFree(c->cloud_ws);
        c->cloud_ws = nullptr; c->cloud_ws_cap = 0;
        HIPCHK(c, hipMalloc(&c->cloud_ws, need));
        c->cloud_ws_cap = need;
    }
    return TDLO_OK;
}

// the one-launch kernels' own workspace for P elements and the pinned words they report through (depth frames and view calls share both, and the state
// words at the workspace's head: a reallocation has them initialised again)
static int ensure_cloud_fws(tdlo_ctx *c, int P) {
    const size_t fneed = cloud_fused_ws_bytes(P);
    if (fneed > c->cloud_fws_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->cloud_fws) hipFree(c->cloud_fws);
        c->cloud_fws = nullptr; c->cloud_fws_cap = 0;
        HIPCHK(c, hipMalloc(&c->cloud_fws, fneed));
        c->cloud_fws_cap = fneed; c->cloud_fused_first = true;
    }
    if (!c->cloud_res) {
        HIPCHK(c, hipHostMalloc((void **)&c->cloud_res, 32 * sizeof(unsigned long long), hipHostMallocDefault));      // [0..1] the report, [4..] phase stamps of an instrumented build
        std::memset(c->cloud_res, 0, 32 * sizeof(unsigned long long));
    }
    return TDLO_OK;
}
// the nodes of a pre-pass that rides in the team kernel: staged in pinned memory, the minima armed
static int stage_vis_ride(tdlo_ctx *c, const double *vis_Y, int vis_M) {
    if (int rc = ensure_vis_state(c)) return rc;
    if (!c->vis_nodes_pin) HIPCHK(c, hipHostMalloc((void **)&c->vis_nodes_pin, sizeof(double) * 3 * 64, hipHostMallocDefault));
    std::memcpy(c->vis_nodes_pin, vis_Y, sizeof(double) * 3 * (size_t)vis_M);
    return TDLO_OK;
}

// pcl/filters/impl/voxel_grid.hpp applyFilter: the leaf-size check and min_b / div_b in float arithmetic from the float bounding box -- the ONE statement
// of the rule for the multi-launch form, whatever its point source (include/trackdlo_hip.h has the contract).  why: what a refusal says.
static int voxel_grid_dims(const float mn[3], const float mx[3], double leaf_size, int min_b[3], int div_b[3], int *nodown, const char **why) {
    const float leaf = (float)leaf_size;
    if (!(leaf > 0.0f) || !std::isfinite(leaf)) { *why = "voxel grid: the leaf size is not a positive finite float"; return TDLO_E_INVALID; }
    for (int d = 0; d < 3; ++d)
        if (!(mn[d] <= mx[d]) || !std::isfinite(mn[d]) || !std::isfinite(mx[d])) { *why = "voxel grid: not a bounding box (min > max, or not finite)"; return TDLO_E_INVALID; }
    const float inv = 1.0f / leaf;
    // "leaf size too small": the exact product dd0 dd1 dd2 > 2^31 - 1, formed stepwise -- every factor is at most 2^31 and the product so far at most
    // 2^31 - 1, so nothing overflows; an extent term that is not a number below 2^31 decides at once
    long long prod = 1;
    bool pass = false;
    for (int d = 0; d < 3 && !pass; ++d) {
        const float ext = (mx[d] - mn[d]) * inv;
        if (!(ext < 2147483648.0f)) { pass = true; break; }
        prod *= (long long)ext + 1;
        if (prod > 2147483647ll) pass = true;
    }
    *nodown = pass ? 1 : 0;
    for (int d = 0; d < 3; ++d) { min_b[d] = 0; div_b[d] = 1; }
    if (pass) return TDLO_OK;
    int mb[3], db[3];
    for (int d = 0; d < 3; ++d) {
        const float lo = std::floor(mn[d] * inv), hi = std::floor(mx[d] * inv);
        const long long dv = (lo >= -2147483648.0f && hi < 2147483648.0f) ? (long long)hi - (long long)lo + 1 : -1;      // (PCL's cast to int is undefined out there)
        if (dv < 1 || dv > 2147483647ll) { *why = "voxel grid: cloud too far from the origin for this leaf size"; return TDLO_E_INVALID; }
        mb[d] = (int)lo; db[d] = (int)dv;
    }
    for (int d = 0; d < 3; ++d) { min_b[d] = mb[d]; div_b[d] = db[d]; }
    return TDLO_OK;
}

int tdlo_voxel_grid_dims(const float mn[3], const float mx[3], double leaf_size, int min_b[3], int div_b[3], int *nodown) {
    if (!mn || !mx || !min_b || !div_b || !nodown) return TDLO_E_INVALID;
    const char *why = nullptr;
    return voxel_grid_dims(mn, mx, leaf_size, min_b, div_b, nodown, &why);
}

// div_b0 div_b1 as the kernels' 32-bit multiplier of ijk2: with fewer than 2^32 - 1 cells a product of 2^31 or more leaves div_b2 = 1, i.e. ijk2 = 0
static int voxel_mul2(const int div_b[3]) { return (int)(unsigned)((long long)div_b[0] * div_b[1]); }

// the grid of a non-empty point set from the box the bounding-box pass left (ordered bits): dims, the cell-count refusal, the radix passes
static int voxel_grid_from_box(tdlo_ctx *c, const unsigned *hb, double leaf_size, int min_b[3], int div_b[3], int *nodown, int *passes) {
    auto decode = [](unsigned o) { const unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o; float f; std::memcpy(&f, &u, 4); return f; };
    float mn[3], mx[3];
    for (int d = 0; d < 3; ++d) { mn[d] = decode(hb[d]); mx[d] = decode(hb[3 + d]); }
    const char *why = nullptr;
    if (int rc = voxel_grid_dims(mn, mx, leaf_size, min_b, div_b, nodown, &why)) return fail(c, rc, why);
    long long cells = 1;                                         // (each factor below 2^31: saturate stepwise)
    for (int d = 0; d < 3; ++d) cells = cells >= 0xffffffffll ? cells : cells * div_b[d];
    if (cells >= 0xffffffffll) return fail(c, TDLO_E_INVALID, "voxel grid has too many cells");
    *passes = 1;
    while (*passes < 4 && (1ll << (8 * *passes)) <= cells) ++*passes;      // every valid key must stay below the all-ones sentinel
    return TDLO_OK;
}

// colour != nullptr (tdlo_colour_*): no mask is handed in -- the frame's segmentation is formed from the colour image, inside the one-launch kernel where
// that serves the frame, else by k_colour_mask into the device mask buffer in front of the mask route
static int depth_to_cloud_impl(tdlo_ctx *c, int slot, const unsigned short *depth, const unsigned char *mask, int rows, int cols,
                               double fx, double fy, double cx, double cy, double leaf_size,
                               double *X_out, int x_capacity, int *n_out, int *n_raw_out, const double *vis_Y, int vis_M, bool *vis_done,
                               const ColourIn *colour = nullptr) {
    if (!c) return TDLO_E_INVALID;
    if (slot < 0 || slot >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
    CloudColour cc{};
    if (colour) {
        if (!colour_pack(colour->params, cc)) return fail(c, TDLO_E_INVALID, "tdlo_colour_params: 1 .. 4 ranges");
        if (!colour->colour) return fail(c, TDLO_E_INVALID, "bad image");
    }
    if (!depth || (!mask && !colour) || rows <= 0 || cols <= 0 || (long long)rows * cols > (1ll << 26)) return fail(c, TDLO_E_INVALID, "bad image");
    if (!(leaf_size > 0) || fx == 0 || fy == 0) return fail(c, TDLO_E_INVALID, "bad leaf size / intrinsics");
    HIPCHK(c, hipSetDevice(c->device));
    Slot &s = c->slots[slot];
    hipStream_t st = c->stream;
    const int P = rows * cols;
    const size_t img = img_depth_bytes(P) + img_mask_bytes(P);
    int rc = ensure_cloud_ws(c, P);
    if (rc) return rc;
    if ((rc = ensure_pin(c, 16))) return rc;
    if (c->cloud_pending >= 0 && (rc = flush_pending_cloud(c))) return rc;      // (a cloud tracking_step staged for this slot is superseded; its copy is harmless and ordered)
    char *base = (char *)c->cloud_ws;
    const unsigned short *d_depth = (unsigned short *)base;
    const unsigned char *d_mask = (unsigned char *)(base + img_depth_bytes(P));
    char *ws = base + img;
    const double cam[4] = {fx, fy, cx, cy};
    // images the caller wrote into the context's pinned buffers (tdlo_image_buffers) are read where they are; anything else is copied first
    const bool in_place = c->img_pin != nullptr && (const char *)depth == c->img_pin && (const char *)mask == c->img_pin + img_depth_bytes(P) &&
                          c->img_pin_rows == rows && c->img_pin_cols == cols;
    bool mask_ready = true;                   // d_mask holds the frame's mask
    if (colour) {
        // the depth image where it is when it lies in the context's pinned buffer, the colour and occluder images likewise (tdlo_colour_buffers); the mask is
        // always the device buffer: k_colour_mask writes it when the one-launch kernel does not serve the frame
        if (c->img_pin != nullptr && (const char *)depth == c->img_pin && c->img_pin_rows == rows && c->img_pin_cols == cols) d_depth = depth;
        else if ((const char *)depth != base) HIPCHK(c, hipMemcpyAsync((void *)d_depth, depth, (size_t)P * 2, hipMemcpyHostToDevice, st));      // (== base: a view call's import wrote it there)
        if ((rc = colour_stage(c, *colour, rows, cols, cc, nullptr))) return rc;
        mask_ready = false;
        if (!(c->colour_fused_on && c->cloud_fused_on && cloud_fused_ok(P))) {
            HIPCHK(c, launch_colour_mask(cc, P, (unsigned char *)d_mask, nullptr, st));
            mask_ready = true; ++c->colour_route[1];
        }
    } else if (in_place) { d_depth = depth; d_mask = mask; }
    else if ((const char *)depth == base && (const char *)mask == base + img_depth_bytes(P)) { }      // a view call's import wrote both there
    else {
        HIPCHK(c, hipMemcpyAsync((void *)d_depth, depth, (size_t)P * 2, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync((void *)d_mask, mask, (size_t)P, hipMemcpyHostToDevice, st));
    }
    if (n_out) *n_out = 0;
    if (n_raw_out) *n_raw_out = 0;
    s.N0 = 0; s.sorted_valid = false;
    const float leaf = (float)leaf_size, inv = 1.0f / leaf;
    int n = -1, nraw = 0;
    if (c->cloud_fused_on && cloud_fused_ok(P)) {
        // ---- one launch (k_cloud_fused); its last workgroup reports through pinned host memory
        if ((rc = ensure_cloud_fws(c, P))) return rc;
        if ((rc = ensure_points(c, s, cloud_fused_max_points()))) return rc;      // (an output point per masked pixel at most; sized once)
        if (++c->cloud_epoch == 0) ++c->cloud_epoch;
        // the frame's visibility pre-pass rides along when the team kernel runs (up to 64 nodes): the nodes staged in pinned memory, read by the kernel
        const bool vis_ride = vis_Y != nullptr && vis_M >= 1 && vis_M <= 64 && c->cloud_team_on && c->direct_in;
        if (vis_ride && (rc = stage_vis_ride(c, vis_Y, vis_M))) return rc;
        HIPCHK(c, launch_cloud_fused(d_depth, d_mask, P, cols, cam, inv, ws, c->cloud_fws, c->cloud_fused_first, c->cloud_team_on, s.Xraw, s.cap_points, c->cloud_res, c->cloud_epoch, st,
                                     vis_ride ? c->vis_nodes_pin : nullptr, vis_ride ? vis_M : 0, c->vis_state, c->vis_res, mask_ready ? nullptr : &cc));
        c->cloud_fused_first = false;
        const int status = cloud_wait(c, st, c->cloud_epoch);
        if (status != 1 && vis_ride) c->vis_armed = false;      // (whatever the team left in the minima: armed again before their next use)
        if (status < 0) { c->cloud_fused_first = true; return status; }
        if (status == 0) { c->cloud_fused_first = true; return fail(c, TDLO_E_HIP, "the stream drained, but the depth -> cloud kernel did not report"); }
        const unsigned long long w1 = __atomic_load_n(c->cloud_res + 1, __ATOMIC_RELAXED);
        nraw = (int)(unsigned)(w1 >> 32);
        if (status == 1 && !mask_ready) ++c->colour_route[0];
        if (status == 1) { n = (int)(unsigned)w1; ++c->cloud_route[0]; if (vis_ride && vis_done) { *vis_done = true; ++c->cloud_vis_rides; } }
        else if (status == 3) return fail(c, TDLO_E_HIP, "voxel grid produced more points than the slot holds");
        else if (status == 4) { c->cloud_fused_first = true; ++c->cloud_route[1]; }      // the team gave the launch up (a wait of 2 s): state words initialised again, the multi-launch form below
        else ++c->cloud_route[1];                 // not taken (too many masked pixels / cells, pass-through): the multi-launch form below
    }
    if (n < 0) {
        if (!mask_ready) {                    // the one-launch kernel passed a colour frame on: its segmentation by the mask kernel, then as for any mask
            HIPCHK(c, launch_colour_mask(cc, P, (unsigned char *)d_mask, nullptr, st));
            mask_ready = true; ++c->colour_route[1];
        }
        // ---- the multi-launch form: bounding box + count, a host round trip, compaction, radix sort passes, centroids
        // the last 64 ints of the workspace: bounding box (6 ordered floats), masked-pixel count, output count
        unsigned *d_bbox = (unsigned *)(ws + cloud_ws_bytes(P) - 256);
        int *d_total = (int *)(d_bbox + 8);
        unsigned *hb = (unsigned *)c->pin;
        hb[0] = hb[1] = hb[2] = ~0u; hb[3] = hb[4] = hb[5] = 0u; hb[6] = 0u; hb[7] = 0u; hb[8] = 0u;
        HIPCHK(c, hipMemcpyAsync(d_bbox, hb, 9 * sizeof(unsigned), hipMemcpyHostToDevice, st));
        HIPCHK(c, launch_cloud_bbox(d_depth, d_mask, P, cols, cam, d_bbox, ws, st));
        HIPCHK(c, hipMemcpyAsync(hb, d_bbox, 8 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        nraw = (int)hb[6];
        if (n_raw_out) *n_raw_out = nraw;
        if (nraw == 0) return TDLO_OK;
        int min_b[3], div_b[3], nodown = 0, passes = 1;
        if ((rc = voxel_grid_from_box(c, hb, leaf_size, min_b, div_b, &nodown, &passes))) return rc;
        rc = ensure_points(c, s, nraw);
        if (rc) return rc;
        HIPCHK(c, launch_cloud_voxels(d_depth, d_mask, P, cols, cam, min_b, div_b[0], voxel_mul2(div_b), inv, nodown, passes, nraw,
                                      ws, d_total, s.cap_points, s.Xraw, st));
        HIPCHK(c, hipMemcpyAsync(hb, d_total, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        n = (int)hb[0];
        if (n < 0 || n > s.cap_points) return fail(c, TDLO_E_HIP, "voxel grid produced an impossible point count");
    }
    if (n_raw_out) *n_raw_out = nraw;
    s.N0 = n; s.sorted_valid = false;
    if (n_out) *n_out = n;
    if (X_out && n > 0) {
        if (n > x_capacity) return fail(c, TDLO_E_INVALID, "X_out too small for the down-sampled cloud");
        HIPCHK(c, hipMemcpyAsync(X_out, s.Xraw, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    return TDLO_OK;
}

int tdlo_depth_to_cloud(tdlo_ctx *c, int slot, const unsigned short *depth, const unsigned char *mask, int rows, int cols,
                        double fx, double fy, double cx, double cy, double leaf_size,
                        double *X_out, int x_capacity, int *n_out, int *n_raw_out) {
    return depth_to_cloud_impl(c, slot, depth, mask, rows, cols, fx, fy, cx, cy, leaf_size, X_out, x_capacity, n_out, n_raw_out, nullptr, 0, nullptr);
}

int tdlo_colour_depth_to_cloud(tdlo_ctx *c, int slot, const unsigned short *depth, const unsigned char *colour, const tdlo_colour_params *params,
                               const unsigned char *occluder, int rows, int cols, double fx, double fy, double cx, double cy, double leaf_size,
                               double *X_out, int x_capacity, int *n_out, int *n_raw_out) {
    const ColourIn ci{colour, params, occluder};
    return depth_to_cloud_impl(c, slot, depth, nullptr, rows, cols, fx, fy, cx, cy, leaf_size, X_out, x_capacity, n_out, n_raw_out, nullptr, 0, nullptr, &ci);
}

// ---- clouds for F slots in one call (include/trackdlo_hip.h: tdlo_depth_to_cloud_batch) ----------------------------------------------------------
// From this many frames on the call is the batch launch; below it loops over the single calls (the same bits).  Set from profiles/cloud_batch_ab.txt by the
// rule "the smallest F from which every batch value lies below every single-calls value, at both image sizes".  Measured: there is no such F up to 32 -- the
// batch wins from pageable images (from 2 frames at 640 x 480, from 3 at 1280 x 720; half the time at 32) and in the tracker call, and by far when frames
// share an image, but F single calls that read the context's pinned image buffers in place stay ahead of a batch that copies caller-pinned images up
// (1.43 against 1.35 ms at 32 frames of 640 x 480 is the batch's only win there; 2.13 against 2.63 ms at 1280 x 720).  So the route is OFF by default (the
// constant lies above any F the measurement covers); TDLO_CLOUD_BATCH_MIN=n, read when the context is made, turns it on from n frames.
constexpr int kCloudBatchMin = 33;

// a batch image's planes: which are in device memory (of the context's GPU)
struct BatchPlanes { bool dev[4] = {false, false, false, false}; };      // depth, mask, colour, occluder

// Everything that refuses the call as a whole; nothing of the context or the slots is touched.  where: per image, where its planes lie.
// The part of it that does not depend on how an image is handed over (packed planes, image views).  image(k): what image k has -- depth, mask, colour,
// fx, fy -- and, behind that, whatever the entrance itself refuses of the image (its planes' locations among it); called for k = 0 .. K - 1 in order.
struct BatchImageHas { bool depth, mask, colour; double fx, fy; };
static int cloud_batch_refusal_common(tdlo_ctx *c, bool have_images, int K, int rows, int cols, const tdlo_batch_frame *frames, int F, double leaf_size,
                                      const std::function<int(int, BatchImageHas &)> &image) {
    if (!have_images || !frames || K < 1 || F < 1) return fail(c, TDLO_E_INVALID, "cloud batch: no images / no frames");
    if (F > (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "cloud batch: more frames than the context has slots");
    if (rows <= 0 || cols <= 0 || (long long)rows * cols > (1ll << 26)) return fail(c, TDLO_E_INVALID, "bad image");
    if (!(leaf_size > 0)) return fail(c, TDLO_E_INVALID, "bad leaf size / intrinsics");
    std::vector<BatchImageHas> has(K);
    for (int k = 0; k < K; ++k)
        if (int rc = image(k, has[k])) return rc;
    for (int f = 0; f < F; ++f) {
        const tdlo_batch_frame &fr = frames[f];
        if (fr.slot < 0 || fr.slot >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
        for (int g = 0; g < f; ++g) if (frames[g].slot == fr.slot) return fail(c, TDLO_E_INVALID, "cloud batch: a slot is named twice");
        if (fr.image < 0 || fr.image >= K) return fail(c, TDLO_E_INVALID, "cloud batch: image index out of range");
        if (fr.colour_params) {
            CloudColour cc;
            if (!colour_pack(fr.colour_params, cc)) return fail(c, TDLO_E_INVALID, "tdlo_colour_params: 1 .. 4 ranges");
            if (!has[fr.image].colour) return fail(c, TDLO_E_INVALID, "cloud batch: colour ranges for an image without a colour image");
        } else if (!has[fr.image].mask) return fail(c, TDLO_E_INVALID, "cloud batch: no colour ranges for an image without a mask");
    }
    return TDLO_OK;
}

static int cloud_batch_refusal(tdlo_ctx *c, const tdlo_batch_image *images, int K, int rows, int cols, const tdlo_batch_frame *frames, int F, double leaf_size,
                               std::vector<BatchPlanes> &where) {
    where.assign(images && K >= 1 ? K : 0, BatchPlanes{});
    return cloud_batch_refusal_common(c, images != nullptr, K, rows, cols, frames, F, leaf_size, [&](int k, BatchImageHas &h) -> int {
        const tdlo_batch_image &im = images[k];
        h = BatchImageHas{im.depth != nullptr, im.mask != nullptr, im.colour != nullptr, im.fx, im.fy};
        if (!im.depth || (!im.mask && !im.colour)) return fail(c, TDLO_E_INVALID, "cloud batch: an image needs depth and a mask or a colour image");
        if (im.fx == 0 || im.fy == 0) return fail(c, TDLO_E_INVALID, "bad leaf size / intrinsics");
        const void *pl[4] = {im.depth, im.mask, im.colour, im.colour ? im.occluder : nullptr};
        for (int q = 0; q < 4; ++q)
            if (pl[q]) { if (int rc = pointer_location(c, pl[q], TDLO_MEM_AUTO, "cloud batch image", &where[k].dev[q])) return rc; }
        return TDLO_OK;
    });
}

// one frame of a batch through the single call (a batch below the crossover, a frame the batch launch passed on): device planes are brought to the host
// first, as the single call takes host images
static int cloud_batch_single(tdlo_ctx *c, const tdlo_batch_image &im, const BatchPlanes &w, const tdlo_batch_frame &fr, int rows, int cols, double leaf_size,
                              int *n_out, int *n_raw_out) {
    const size_t P = (size_t)rows * cols;
    std::vector<unsigned char> hold[4];
    auto host = [&](const void *p, int q, size_t bytes, const void **out) -> int {
        *out = p;
        if (!p || !w.dev[q]) return TDLO_OK;
        hold[q].resize(bytes);
        HIPCHK(c, hipMemcpy(hold[q].data(), p, bytes, hipMemcpyDeviceToHost));
        *out = hold[q].data();
        return TDLO_OK;
    };
    const void *d = nullptr, *m = nullptr, *col = nullptr, *occ = nullptr;
    int rc = host(im.depth, 0, 2 * P, &d);
    if (rc) return rc;
    if (!fr.colour_params) {
        if ((rc = host(im.mask, 1, P, &m))) return rc;
        return depth_to_cloud_impl(c, fr.slot, (const unsigned short *)d, (const unsigned char *)m, rows, cols, im.fx, im.fy, im.cx, im.cy, leaf_size, nullptr, 0, n_out,
                                   n_raw_out, nullptr, 0, nullptr);
    }
    if ((rc = host(im.colour, 2, 3 * P, &col)) || (rc = host(im.occluder, 3, P, &occ))) return rc;
    const ColourIn ci{(const unsigned char *)col, fr.colour_params, (const unsigned char *)occ};
    return depth_to_cloud_impl(c, fr.slot, (const unsigned short *)d, nullptr, rows, cols, im.fx, im.fy, im.cx, im.cy, leaf_size, nullptr, 0, n_out, n_raw_out, nullptr, 0,
                               nullptr, &ci);
}

// What the batch entrances share (tdlo_depth_to_cloud_batch: packed images; tdlo_frame_views_to_cloud_batch: image views): the arena, the arming of the
// state words, the descriptor table, the launches' place on the stream, the one host wait and the result words.  A frame as this part sees it: its slot,
// where its canonical planes lie in the arena's plane region (byte offsets; kNoPlane: none), its colour ranges (nullptr: the mask) and its camera.
constexpr size_t kNoPlane = ~(size_t)0;
struct CloudBatchIn { int slot; size_t depth, mask, colour, occluder; const tdlo_colour_params *cp; double cam[4]; };
// the arena of one call: [descriptor table | the entrance's second table (tab2 bytes, may be none) | plane region] in device memory; the same two tables and
// `tail` bytes of the entrance's own behind them in pinned memory
struct CloudBatchArena { char *d_tab, *d_tab2, *d_img, *h_tab, *h_tab2, *h_tail; };
// What an entrance does between the armed arena and the host wait, all on the context's stream: bring the planes into the plane region, upload the table(s),
// launch.  bf: the frames in launch order (Fm that bring a mask, then Fc that form it from colour), ready for launch_cloud_fused_batch / cloud_fused_batch_table
using CloudBatchEnqueue = std::function<int(const CloudBatchArena &, const CloudBatchFrame *bf, int Fm, int Fc, float inv_leaf, unsigned epoch)>;

// the arena's table-and-plane block in device memory and its pinned block, grown on demand (the cloud batch's entrances and the rig calls: whoever comes
// next writes both from their start)
static int ensure_batch_arena(tdlo_ctx *c, size_t dev_bytes, size_t pin_bytes) {
    hipStream_t st = c->stream;
    if (dev_bytes > c->cbat_img_cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->cbat_img) hipFree(c->cbat_img);
        c->cbat_img = nullptr; c->cbat_img_cap = 0;
        HIPCHK(c, hipMalloc(&c->cbat_img, dev_bytes));
        c->cbat_img_cap = dev_bytes;
    }
    if (pin_bytes > c->cbat_pin_cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->cbat_pin) hipHostFree(c->cbat_pin);
        c->cbat_pin = nullptr; c->cbat_pin_cap = 0;
        HIPCHK(c, hipHostMalloc((void **)&c->cbat_pin, pin_bytes, hipHostMallocDefault));
        std::memset(c->cbat_pin, 0, pin_bytes);
        c->cbat_pin_cap = pin_bytes;
    }
    return TDLO_OK;
}

// the packed planes a call brings into the arena's plane region: every distinct (pointer, kind) once -- kind: 0 depth, 1 mask, 2 colour, 3 occluder -- each in
// a padded place of its own (the kernels' loads run up to 16 bytes beyond an image); device planes are copied device to device
struct BatchPlaneSet {
    struct Plane { const void *src; int kind; size_t off; bool dev; };
    std::vector<Plane> planes;
    size_t bytes = 0;
    size_t add(const void *src, int kind, bool dev, size_t P) {      // the plane's byte offset in the plane region
        size_t j = 0;
        while (j < planes.size() && !(planes[j].src == src && planes[j].kind == kind)) ++j;
        if (j == planes.size()) {
            planes.push_back(Plane{src, kind, bytes, dev});
            bytes += kind == 0 ? img_depth_bytes(P) : kind == 1 ? img_mask_bytes(P) : kind == 2 ? img_colour_bytes(P) : img_occ_bytes(P);
        }
        return planes[j].off;
    }
};
static int batch_planes_copy(tdlo_ctx *c, const BatchPlaneSet &set, char *d_img, size_t P) {
    const size_t plane_copy[4] = {2 * P, P, 3 * P, P};
    for (const BatchPlaneSet::Plane &pl : set.planes)
        HIPCHK(c, hipMemcpyAsync(d_img + pl.off, pl.src, plane_copy[pl.kind], pl.dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    return TDLO_OK;
}

// route: the entrance's two counters (frames served / passed on).  passed: the frames the kernel did not take, for the entrance's single route.
static int cloud_batch_run(tdlo_ctx *c, const std::vector<CloudBatchIn> &in, int P, double leaf_size, size_t tab2, size_t img_bytes, size_t tail,
                           const CloudBatchEnqueue &enqueue, long long *route, std::vector<int> &n, std::vector<int> &nraw, std::vector<int> &rcs, std::vector<int> &passed) {
    const int F = (int)in.size();
    int rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (c->cloud_pending >= 0 && (rc = flush_pending_cloud(c))) return rc;
    c->fvbat_planes.clear();                                  // (tdlo_view_batch_images: the arena is about to be written)
    // ---- the arena: F frame blocks; the table(s) and the planes of the images in use
    auto r256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t fb = cloud_batch_frame_bytes(P), tab = r256(cloud_batch_desc_bytes() * (size_t)F);
    // (two device blocks: a frame block's place must not depend on what else a call brings -- its state words stay armed from call to call -- so the table
    // and the planes, whose sizes change with every call, live apart from the frame blocks)
    if (fb * (size_t)F > c->cbat_dev_cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->cbat_dev) hipFree(c->cbat_dev);
        c->cbat_dev = nullptr; c->cbat_dev_cap = 0; c->cbat_armed_F = 0;
        HIPCHK(c, hipMalloc(&c->cbat_dev, fb * (size_t)F));
        c->cbat_dev_cap = fb * (size_t)F;
    }
    if ((rc = ensure_batch_arena(c, tab + tab2 + img_bytes, 2 * sizeof(unsigned long long) * (size_t)F + tab + tab2 + tail))) return rc;
    char *base = (char *)c->cbat_dev;
    unsigned long long *res = (unsigned long long *)c->cbat_pin;
    CloudBatchArena ar;
    ar.d_tab = (char *)c->cbat_img; ar.d_tab2 = ar.d_tab + tab; ar.d_img = ar.d_tab2 + tab2;
    ar.h_tab = c->cbat_pin + 2 * sizeof(unsigned long long) * (size_t)F; ar.h_tab2 = ar.h_tab + tab; ar.h_tail = ar.h_tab2 + tab2;
    std::memset(res, 0, 2 * sizeof(unsigned long long) * (size_t)F);      // (where another F had its table: no word may look like this call's epoch)
    // ---- the slots: room for a point per masked pixel the kernel takes; whatever was resident is gone from here on
    for (int f = 0; f < F; ++f) {
        Slot &s = c->slots[in[f].slot];
        if ((rc = ensure_points(c, s, cloud_fused_max_points()))) return rc;
        s.N0 = 0; s.sorted_valid = false;
    }
    // ---- state words
    if (c->cbat_armed_P != P || F > c->cbat_armed_F) {
        std::vector<void *> blocks(F);
        for (int f = 0; f < F; ++f) blocks[f] = base + fb * (size_t)f;
        c->cbat_armed_F = 0;
        HIPCHK(c, cloud_batch_arm(blocks.data(), F, P, st));
        c->cbat_armed_F = F; c->cbat_armed_P = P;
    }
    // ---- the table: the frames that bring a mask, then the frames that form it from the colour image
    std::vector<int> order;
    for (int f = 0; f < F; ++f) if (!in[f].cp) order.push_back(f);
    const int Fm = (int)order.size();
    for (int f = 0; f < F; ++f) if (in[f].cp) order.push_back(f);
    std::vector<CloudBatchFrame> bf(F);
    for (int j = 0; j < F; ++j) {
        const CloudBatchIn &fr = in[order[j]];
        CloudBatchFrame &b = bf[j];
        b = CloudBatchFrame{};
        b.depth = (const unsigned short *)(ar.d_img + fr.depth);
        if (fr.cp) {
            colour_pack(fr.cp, b.colour);
            b.colour.colour = (const unsigned char *)(ar.d_img + fr.colour);
            b.colour.occluder = fr.occluder != kNoPlane ? (const unsigned char *)(ar.d_img + fr.occluder) : nullptr;
        } else b.mask = (const unsigned char *)(ar.d_img + fr.mask);
        for (int q = 0; q < 4; ++q) b.cam[q] = fr.cam[q];
        b.ws = base + fb * (size_t)j;
        Slot &s = c->slots[fr.slot];
        b.X = s.Xraw; b.cap = s.cap_points; b.res = res + 2 * (size_t)j;
    }
    if (++c->cloud_epoch == 0) ++c->cloud_epoch;
    const unsigned epoch = c->cloud_epoch;
    const float leaf = (float)leaf_size, inv = 1.0f / leaf;
    // ---- the planes, the table(s), the launches: the entrance's
    if ((rc = enqueue(ar, bf.data(), Fm, F - Fm, inv, epoch))) { c->cbat_armed_F = 0; return rc; }
    {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) { c->cbat_armed_F = 0; HIPCHK(c, e); }
    }
    // ---- the frames' words; a frame the kernel did not take goes through the single call for its slot alone
    for (int j = 0; j < F; ++j) {
        const int f = order[j];
        const unsigned long long w0 = __atomic_load_n(res + 2 * (size_t)j, __ATOMIC_ACQUIRE), w1 = __atomic_load_n(res + 2 * (size_t)j + 1, __ATOMIC_RELAXED);
        const unsigned status = (unsigned)w0;
        if ((unsigned)(w0 >> 32) != epoch) { c->cbat_armed_F = 0; rcs[f] = fail(c, TDLO_E_HIP, "the stream drained, but a frame of the depth -> cloud batch did not report"); continue; }
        nraw[f] = (int)(unsigned)(w1 >> 32);
        if (status == 1u) { n[f] = (int)(unsigned)w1; c->slots[in[f].slot].N0 = n[f]; ++route[0]; }
        else if (status == 2u) { passed.push_back(f); ++route[1]; }
        else rcs[f] = fail(c, TDLO_E_HIP, "voxel grid produced more points than the slot holds");
    }
    return TDLO_OK;
}

int tdlo_depth_to_cloud_batch(tdlo_ctx *c, const tdlo_batch_image *images, int K, int rows, int cols, const tdlo_batch_frame *frames, int F, double leaf_size,
                              int *n_out, int *n_raw_out, int *rc_each) {
    if (!c) return TDLO_E_INVALID;
    std::vector<BatchPlanes> where;
    int rc = cloud_batch_refusal(c, images, K, rows, cols, frames, F, leaf_size, where);
    if (rc) return rc;
    std::vector<int> n(F, 0), nraw(F, 0), rcs(F, 0);
    auto finish = [&]() {
        if (n_out) std::copy(n.begin(), n.end(), n_out);
        if (n_raw_out) std::copy(nraw.begin(), nraw.end(), n_raw_out);
        if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
        for (int f = 0; f < F; ++f) if (rcs[f]) return rcs[f];
        return (int)TDLO_OK;
    };
    const int P = rows * cols;
    if (F < (c->cloud_batch_min ? c->cloud_batch_min : kCloudBatchMin) || !c->cloud_fused_on || !cloud_fused_ok(P)) {
        for (int f = 0; f < F; ++f)
            rcs[f] = cloud_batch_single(c, images[frames[f].image], where[frames[f].image], frames[f], rows, cols, leaf_size, &n[f], &nraw[f]);
        return finish();
    }
    // ---- the planes of the images in use
    std::vector<char> use(4 * (size_t)K, 0);                  // plane q of image k is read by a frame
    for (int f = 0; f < F; ++f) {
        const int k = frames[f].image;
        use[4 * k] = 1;
        if (frames[f].colour_params) { use[4 * k + 2] = 1; if (images[k].occluder) use[4 * k + 3] = 1; }
        else use[4 * k + 1] = 1;
    }
    BatchPlaneSet planes;                                     // every distinct (pointer, kind) once
    std::vector<size_t> at(4 * (size_t)K, 0);
    for (int k = 0; k < K; ++k) {
        const void *pl[4] = {images[k].depth, images[k].mask, images[k].colour, images[k].occluder};
        for (int q = 0; q < 4; ++q)
            if (use[4 * k + q]) at[4 * k + q] = planes.add(pl[q], q, where[k].dev[q], (size_t)P);
    }
    const size_t img_bytes = planes.bytes;
    std::vector<CloudBatchIn> in(F);
    for (int f = 0; f < F; ++f) {
        const int k = frames[f].image;
        const tdlo_batch_image &im = images[k];
        in[f] = CloudBatchIn{frames[f].slot, at[4 * k], at[4 * k + 1], at[4 * k + 2], im.occluder ? at[4 * k + 3] : kNoPlane, frames[f].colour_params, {im.fx, im.fy, im.cx, im.cy}};
    }
    hipStream_t st = c->stream;
    const CloudBatchEnqueue enqueue = [&](const CloudBatchArena &ar, const CloudBatchFrame *bf, int Fm, int Fc, float inv, unsigned epoch) -> int {
        // every distinct plane once (device planes device to device: the kernel's loads want the padding behind the image)
        if (int rcp = batch_planes_copy(c, planes, ar.d_img, (size_t)P)) return rcp;
        HIPCHK(c, launch_cloud_fused_batch(bf, Fm, Fc, P, cols, inv, epoch, ar.h_tab, ar.d_tab, st));
        return TDLO_OK;
    };
    std::vector<int> passed;
    if ((rc = cloud_batch_run(c, in, P, leaf_size, 0, img_bytes, 0, enqueue, c->cbat_route, n, nraw, rcs, passed))) return rc;
    for (int f : passed)
        rcs[f] = cloud_batch_single(c, images[frames[f].image], where[frames[f].image], frames[f], rows, cols, leaf_size, &n[f], &nraw[f]);
    return finish();
}

// ---- the voxel grid on a cloud view (include/trackdlo_hip.h: V(view, N, select, leaf)) ---------------------------------------------------------
// Everything that can refuse the call without a look at the points; nothing of the context or the slot is touched.
static int voxel_view_refusal(tdlo_ctx *c, int slot, const tdlo_cloud_view *v, int N, double leaf_size) {
    if (const char *why = view_fault(v, N)) return fail(c, TDLO_E_INVALID, why);
    if (slot < 0 || slot >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
    if (v->flags & TDLO_VIEW_ASYNC) return fail(c, TDLO_E_INVALID, "voxel grid on a view: TDLO_VIEW_ASYNC is not available (the call reads the bounding box back)");
    if (N > (1 << 26)) return fail(c, TDLO_E_INVALID, "voxel grid on a view: more than 2^26 points");
    const float leaf = (float)leaf_size;
    if (!(leaf > 0.0f) || !std::isfinite(leaf)) return fail(c, TDLO_E_INVALID, "voxel grid: the leaf size is not a positive finite float");
    return TDLO_OK;
}

// vis_Y != nullptr: the caller wants the frame's visibility pre-pass as well; *vis_done = true when the team kernel has left the M squared minima in
// c->vis_res[1 ..], as for depth_to_cloud_impl
static int cloud_view_voxel_impl(tdlo_ctx *c, int slot, const tdlo_cloud_view *v, int N, const unsigned char *select, double leaf_size,
                                 double *X_out, int x_capacity, int *n_out, int *n_raw_out, const double *vis_Y, int vis_M, bool *vis_done) {
    if (!c) return TDLO_E_INVALID;
    int rc = voxel_view_refusal(c, slot, v, N, leaf_size);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    bool device = false, sel_device = false;
    if ((rc = view_location(c, v, &device))) return rc;
    if (select && (rc = pointer_location(c, select, TDLO_MEM_AUTO, "select", &sel_device))) return rc;
    Slot &s = c->slots[slot];
    const bool f64 = v->dtype == TDLO_F64;
    if (device && s.Xraw) {                                      // the centroids are written while the view is still being read
        long long lo = 0, hi = 0;
        (void)tdlo_cloud_view_extent(v, N, &lo, &hi);
        const char *a0 = (const char *)v->data + lo, *a1 = (const char *)v->data + hi;
        const char *x0 = (const char *)s.Xraw, *x1 = x0 + 3 * (size_t)s.cap_points * sizeof(double);
        if (a0 < x1 && x0 < a1) return fail(c, TDLO_E_INVALID, "voxel grid on a view: the view aliases the slot's resident cloud");
    }
    hipStream_t st = c->stream;
    if ((rc = ensure_cloud_ws(c, N)) || (rc = ensure_pin(c, 16)) || (rc = flush_pending_cloud(c))) return rc;
    char *base = (char *)c->cloud_ws;
    char *ws = base + img_depth_bytes(N) + img_mask_bytes(N);
    CloudViewSrc src{v->data, f64, v->stride_point, v->stride_comp, select};
    if (device) {
        if (v->ready_stream) {
            if (!c->ev_view) HIPCHK(c, hipEventCreateWithFlags(&c->ev_view, hipEventDisableTiming));
            HIPCHK(c, hipEventRecord(c->ev_view, (hipStream_t)v->ready_stream));
            HIPCHK(c, hipStreamWaitEvent(st, c->ev_view, 0));
        }
    } else {
        // a host view: packed column-major in its own precision into the pinned staging block, which the kernels read in place (the bounding-box and key
        // passes once each, the centroid pass the kept points)
        const size_t bytes = 3 * (size_t)N * (f64 ? 8 : 4);
        if ((rc = ensure_cloud_pin(c, (bytes + 7) / 8))) return rc;
        if (f64) view_gather((double *)c->cloud_pin, (const double *)v->data, v->stride_point, v->stride_comp, N);
        else view_gather((float *)c->cloud_pin, (const float *)v->data, v->stride_point, v->stride_comp, N);
        src.data = c->cloud_pin; src.stride_point = 1; src.stride_comp = N;
    }
    if (select && !sel_device) {                                 // host selection bytes: to the context's device mask buffer
        unsigned char *d_mask = (unsigned char *)(base + img_depth_bytes(N));
        HIPCHK(c, hipMemcpyAsync(d_mask, select, (size_t)N, hipMemcpyHostToDevice, st));
        src.select = d_mask;
    }
    ++c->voxel_view_calls;
    const float inv = 1.0f / (float)leaf_size;
    if (c->cloud_fused_on && c->cloud_team_on && cloud_fused_ok(N)) {
        // ---- one launch (k_cloud_team over the view; TDLO_CLOUD_FUSED=0 / TDLO_CLOUD_TEAM=0: the multi-launch form below, the comparator).  The kernel
        // decides whether it serves the call: more than 32 704 kept points, pass-through, too many cell bits and every case that refuses the call go on to
        // the multi-launch form, which decides them.  It is launched with the slot's capacity AS IT IS -- growing the slot frees its resident cloud, which a
        // refusal must leave intact -- and writes nothing to the slot unless the result fits: "capacity" too goes on, to the code that grows the slot
        if ((rc = ensure_cloud_fws(c, N))) return rc;
        if (++c->cloud_epoch == 0) ++c->cloud_epoch;
        const bool vis_ride = vis_Y != nullptr && vis_M >= 1 && vis_M <= 64 && c->direct_in;
        if (vis_ride && (rc = stage_vis_ride(c, vis_Y, vis_M))) return rc;
        HIPCHK(c, launch_view_team(src, N, inv, ws, c->cloud_fws, c->cloud_fused_first, s.Xraw, s.cap_points, c->cloud_res, c->cloud_epoch, st,
                                   vis_ride ? c->vis_nodes_pin : nullptr, vis_ride ? vis_M : 0, c->vis_state, c->vis_res));
        c->cloud_fused_first = false;
        const int status = cloud_wait(c, st, c->cloud_epoch);
        if (status != 1 && vis_ride) c->vis_armed = false;      // (whatever the team left in the minima: armed again before their next use)
        if (status < 0) { c->cloud_fused_first = true; return status; }
        if (status == 0) { c->cloud_fused_first = true; return fail(c, TDLO_E_HIP, "the stream drained, but the voxel-grid kernel did not report"); }
        if (status == 1) {
            const unsigned long long w1 = __atomic_load_n(c->cloud_res + 1, __ATOMIC_RELAXED);
            const int n = (int)(unsigned)w1, nraw = (int)(unsigned)(w1 >> 32);
            ++c->view_team_route[0];
            if (n < 0 || n > s.cap_points || n > nraw) return fail(c, TDLO_E_HIP, "voxel grid produced an impossible point count");
            s.N0 = n; s.sorted_valid = false;                   // (nraw == 0: n = 0, the slot as tdlo_depth_to_cloud leaves it for an all-zero mask)
            if (n_out) *n_out = n;
            if (n_raw_out) *n_raw_out = nraw;
            if (n > 0 && vis_ride && vis_done) { *vis_done = true; ++c->view_team_route[2]; }
            if (X_out && n > 0) {
                if (n > x_capacity) return fail(c, TDLO_E_INVALID, "X_out too small for the down-sampled cloud");
                HIPCHK(c, hipMemcpyAsync(X_out, s.Xraw, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipStreamSynchronize(st));
            }
            return TDLO_OK;
        }
        if (status == 4) c->cloud_fused_first = true;           // the team gave the launch up (a wait of 2 s): state words initialised again
        ++c->view_team_route[1];                                 // passed on: not taken (2), the slot has to grow first (3), given up (4)
    }
    // ---- the multi-launch form: bounding box + count, a host round trip, compaction, radix sort passes, centroids
    unsigned *d_bbox = (unsigned *)(ws + cloud_ws_bytes(N) - 256);
    int *d_total = (int *)(d_bbox + 8);
    unsigned *hb = (unsigned *)c->pin;
    hb[0] = hb[1] = hb[2] = ~0u; hb[3] = hb[4] = hb[5] = 0u; hb[6] = 0u; hb[7] = 0u; hb[8] = 0u;
    HIPCHK(c, hipMemcpyAsync(d_bbox, hb, 9 * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIPCHK(c, launch_view_bbox(src, N, d_bbox, ws, st));
    HIPCHK(c, hipMemcpyAsync(hb, d_bbox, 8 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const int nraw = (int)hb[6];
    if (n_out) *n_out = 0;
    if (n_raw_out) *n_raw_out = nraw;
    if (nraw == 0) { s.N0 = 0; s.sorted_valid = false; return TDLO_OK; }      // the slot as tdlo_depth_to_cloud leaves it for an all-zero mask
    int min_b[3], div_b[3], nodown = 0, passes = 1;
    if ((rc = voxel_grid_from_box(c, hb, leaf_size, min_b, div_b, &nodown, &passes))) return rc;      // (the slot's cloud is untouched)
    if ((rc = ensure_points(c, s, nraw))) return rc;
    s.N0 = 0; s.sorted_valid = false;
    HIPCHK(c, launch_view_voxels(src, N, min_b, div_b[0], voxel_mul2(div_b), inv, nodown, passes, nraw, ws, d_total, s.cap_points, s.Xraw, st));
    HIPCHK(c, hipMemcpyAsync(hb, d_total, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const int n = (int)hb[0];
    if (n < 0 || n > s.cap_points) return fail(c, TDLO_E_HIP, "voxel grid produced an impossible point count");
    s.N0 = n;
    if (n_out) *n_out = n;
    if (X_out && n > 0) {
        if (n > x_capacity) return fail(c, TDLO_E_INVALID, "X_out too small for the down-sampled cloud");
        HIPCHK(c, hipMemcpyAsync(X_out, s.Xraw, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    return TDLO_OK;
}

int tdlo_cloud_view_voxel_grid(tdlo_ctx *c, int slot, const tdlo_cloud_view *v, int N, const unsigned char *select, double leaf_size,
                               double *X_out, int x_capacity, int *n_out, int *n_raw_out) {
    return cloud_view_voxel_impl(c, slot, v, N, select, leaf_size, X_out, x_capacity, n_out, n_raw_out, nullptr, 0, nullptr);
}

// ---- one cloud from several cameras (include/trackdlo_hip.h: the rig's point list R, then V(R, leaf)) ------------------------------------------------------
// Everything that refuses the call as a whole; nothing of the context or the slot is touched.  dev: per camera, which of its planes (depth, mask, colour,
// occluder) lie in device memory
static int rig_refusal(tdlo_ctx *c, int slot, const tdlo_rig_camera *cams, int K, int rows, int cols, double leaf_size, std::vector<BatchPlanes> &dev) {
    if (slot < 0 || slot >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
    if (const char *why = rig_fault(cams, K, rows, cols, leaf_size)) return fail(c, TDLO_E_INVALID, why);
    dev.assign(K, BatchPlanes{});
    for (int k = 0; k < K; ++k) {
        const bool colour = rig_camera_colour(cams[k]);
        const void *pl[4] = {cams[k].depth, colour ? nullptr : cams[k].mask, colour ? cams[k].colour : nullptr, colour ? cams[k].occluder : nullptr};
        for (int q = 0; q < 4; ++q)
            if (pl[q]) { if (int rc = pointer_location(c, pl[q], TDLO_MEM_AUTO, "rig camera", &dev[k].dev[q])) return rc; }
    }
    return TDLO_OK;
}

// vis_Y != nullptr: the caller wants the frame's visibility pre-pass as well; *vis_done = true when the team kernel has left the M squared minima in
// c->vis_res[1 ..], as for cloud_view_voxel_impl -- whose result words, epoch, riding pre-pass and hand-over these are
static int rig_to_cloud_impl(tdlo_ctx *c, int slot, const tdlo_rig_camera *cams, int K, int rows, int cols, double leaf_size,
                             double *X_out, int x_capacity, int *n_out, int *n_raw_out, const double *vis_Y, int vis_M, bool *vis_done) {
    if (!c) return TDLO_E_INVALID;
    std::vector<BatchPlanes> where;
    int rc = rig_refusal(c, slot, cams, K, rows, cols, leaf_size, where);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Slot &s = c->slots[slot];
    hipStream_t st = c->stream;
    const int P = rows * cols, Tc = rig_tiles_per_camera(P);
    const bool colour = rig_camera_colour(cams[0]);
    const int E = K * Tc * kRigTile;                             // elements of the one-launch form's tile regions (K P <= 2^26: below 2^27)
    // ---- the arena (the cloud batch's device block and pinned block, by its helpers): [camera table | every distinct plane once | a colour rig's K mask planes]
    auto r256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    BatchPlaneSet planes;
    std::vector<size_t> at(4 * (size_t)K, kNoPlane);
    const size_t tab = r256(rig_table_bytes(K));
    for (int k = 0; k < K; ++k) {
        const void *pl[4] = {cams[k].depth, colour ? nullptr : cams[k].mask, colour ? cams[k].colour : nullptr, colour ? cams[k].occluder : nullptr};
        for (int q = 0; q < 4; ++q)
            if (pl[q]) at[4 * k + q] = planes.add(pl[q], q, where[k].dev[q], (size_t)P);
    }
    const size_t masks_at = planes.bytes, mask_bytes = img_mask_bytes(P);
    const size_t img_bytes = planes.bytes + (colour ? mask_bytes * (size_t)K : 0);
    for (const BatchPlaneSet::Plane &pl : planes.planes) {        // (a device plane is copied device to device: it must not lie in the arena itself)
        const size_t len = (pl.kind == 0 ? 2 : pl.kind == 2 ? 3 : 1) * (size_t)P;
        if (pl.dev && c->cbat_img && (const char *)pl.src < (const char *)c->cbat_img + c->cbat_img_cap && (const char *)c->cbat_img < (const char *)pl.src + len)
            return fail(c, TDLO_E_INVALID, "rig: a device plane overlaps the batch arena");
    }
    if ((rc = ensure_cloud_ws(c, E)) || (rc = ensure_pin(c, 16)) || (rc = flush_pending_cloud(c))) return rc;
    c->fvbat_planes.clear();                                      // (tdlo_view_batch_images: the arena is about to be written)
    if ((rc = ensure_batch_arena(c, tab + img_bytes, tab))) return rc;
    char *d_tab = (char *)c->cbat_img, *d_img = d_tab + tab;
    if ((rc = batch_planes_copy(c, planes, d_img, (size_t)P))) return rc;
    // ---- the camera table goes up with the launch, as the batch tables do
    RigCam *h_tab = (RigCam *)c->cbat_pin;
    for (int k = 0; k < K; ++k) {
        RigCam &r = h_tab[k];
        rig_camera_record(cams[k], r);
        r.depth = (const unsigned short *)(d_img + at[4 * k]);
        r.mask = (const unsigned char *)(d_img + (colour ? masks_at + mask_bytes * (size_t)k : at[4 * k + 1]));
        r.colour = colour ? (const unsigned char *)(d_img + at[4 * k + 2]) : nullptr;
        r.occluder = colour && at[4 * k + 3] != kNoPlane ? (const unsigned char *)(d_img + at[4 * k + 3]) : nullptr;
    }
    HIPCHK(c, hipMemcpyAsync(d_tab, h_tab, rig_table_bytes(K), hipMemcpyHostToDevice, st));
    char *ws = (char *)c->cloud_ws + img_depth_bytes(E) + img_mask_bytes(E);
    const float inv = 1.0f / (float)leaf_size;
    if (c->cloud_fused_on && c->cloud_team_on && (long long)K * Tc <= 4095) {
        // ---- one launch (k_cloud_team over the rig).  As for a view: launched with the slot's capacity AS IT IS where a cloud is resident -- growing the slot
        // frees that cloud, which a refusal must leave intact -- and the kernel writes nothing to the slot unless the result fits; an empty slot is sized first
        if ((rc = ensure_cloud_fws(c, E))) return rc;
        if (s.N0 == 0 && (rc = ensure_points(c, s, cloud_fused_max_points()))) return rc;
        if (++c->cloud_epoch == 0) ++c->cloud_epoch;
        const bool vis_ride = vis_Y != nullptr && vis_M >= 1 && vis_M <= 64 && c->direct_in;
        if (vis_ride && (rc = stage_vis_ride(c, vis_Y, vis_M))) return rc;
        HIPCHK(c, launch_rig_team(d_tab, K, P, cols, colour, inv, ws, c->cloud_fws, c->cloud_fused_first, s.Xraw, s.cap_points, c->cloud_res, c->cloud_epoch, st,
                                  vis_ride ? c->vis_nodes_pin : nullptr, vis_ride ? vis_M : 0, c->vis_state, c->vis_res));
        c->cloud_fused_first = false;
        const int status = cloud_wait(c, st, c->cloud_epoch);
        if (status != 1 && vis_ride) c->vis_armed = false;      // (whatever the team left in the minima: armed again before their next use)
        if (status < 0) { c->cloud_fused_first = true; return status; }
        if (status == 0) { c->cloud_fused_first = true; return fail(c, TDLO_E_HIP, "the stream drained, but the rig kernel did not report"); }
        if (status == 1) {
            const unsigned long long w1 = __atomic_load_n(c->cloud_res + 1, __ATOMIC_RELAXED);
            const int n = (int)(unsigned)w1, nraw = (int)(unsigned)(w1 >> 32);
            ++c->rig_route[0];
            if (n < 0 || n > s.cap_points || n > nraw) return fail(c, TDLO_E_HIP, "voxel grid produced an impossible point count");
            s.N0 = n; s.sorted_valid = false;
            if (n_out) *n_out = n;
            if (n_raw_out) *n_raw_out = nraw;
            if (n > 0 && vis_ride && vis_done) { *vis_done = true; ++c->rig_route[2]; }
            if (X_out && n > 0) {
                if (n > x_capacity) return fail(c, TDLO_E_INVALID, "X_out too small for the down-sampled cloud");
                HIPCHK(c, hipMemcpyAsync(X_out, s.Xraw, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipStreamSynchronize(st));
            }
            return TDLO_OK;
        }
        if (status == 4) c->cloud_fused_first = true;           // the team gave the launch up (a wait of 2 s): state words initialised again
    }
    ++c->rig_route[1];               // passed on -- by the kernel: not taken (2), the slot has to grow first (3), given up (4); by the host: tiles, switches
    // ---- the multi-launch form over K P elements (element p: camera p / P, pixel p % P): a colour rig's masks first, per camera, into the arena
    if (colour)
        for (int k = 0; k < K; ++k) {
            CloudColour cc{};
            (void)colour_pack(cams[k].colour_params, cc);
            cc.colour = h_tab[k].colour; cc.occluder = h_tab[k].occluder;
            HIPCHK(c, launch_colour_mask(cc, P, (unsigned char *)h_tab[k].mask, nullptr, st));
        }
    const int N = K * P;
    unsigned *d_bbox = (unsigned *)(ws + cloud_ws_bytes(N) - 256);
    int *d_total = (int *)(d_bbox + 8);
    unsigned *hb = (unsigned *)c->pin;
    hb[0] = hb[1] = hb[2] = ~0u; hb[3] = hb[4] = hb[5] = 0u; hb[6] = 0u; hb[7] = 0u; hb[8] = 0u;
    HIPCHK(c, hipMemcpyAsync(d_bbox, hb, 9 * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIPCHK(c, launch_rig_bbox(d_tab, K, P, cols, d_bbox, ws, st));
    HIPCHK(c, hipMemcpyAsync(hb, d_bbox, 8 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const int nraw = (int)hb[6];
    if (n_out) *n_out = 0;
    if (n_raw_out) *n_raw_out = nraw;
    if (nraw == 0) { s.N0 = 0; s.sorted_valid = false; return TDLO_OK; }      // the slot as tdlo_depth_to_cloud leaves it for an all-zero mask
    int min_b[3], div_b[3], nodown = 0, passes = 1;
    if ((rc = voxel_grid_from_box(c, hb, leaf_size, min_b, div_b, &nodown, &passes))) return rc;      // (the slot's cloud is untouched)
    if ((rc = ensure_points(c, s, nraw))) return rc;
    s.N0 = 0; s.sorted_valid = false;
    HIPCHK(c, launch_rig_voxels(d_tab, K, P, cols, min_b, div_b[0], voxel_mul2(div_b), inv, nodown, passes, nraw, ws, d_total, s.cap_points, s.Xraw, st));
    HIPCHK(c, hipMemcpyAsync(hb, d_total, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const int n = (int)hb[0];
    if (n < 0 || n > s.cap_points) return fail(c, TDLO_E_HIP, "voxel grid produced an impossible point count");
    s.N0 = n;
    if (n_out) *n_out = n;
    if (X_out && n > 0) {
        if (n > x_capacity) return fail(c, TDLO_E_INVALID, "X_out too small for the down-sampled cloud");
        HIPCHK(c, hipMemcpyAsync(X_out, s.Xraw, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    return TDLO_OK;
}

int tdlo_rig_to_cloud(tdlo_ctx *c, int slot, const tdlo_rig_camera *cams, int K, int rows, int cols, double leaf_size,
                      double *X_out, int x_capacity, int *n_out, int *n_raw_out) {
    return rig_to_cloud_impl(c, slot, cams, K, rows, cols, leaf_size, X_out, x_capacity, n_out, n_raw_out, nullptr, 0, nullptr);
}

// ---- rigs for F slots in one call (include/trackdlo_hip.h: tdlo_rig_to_cloud_batch, tdlo_tracker_frames_from_rig_batch) ---------------------------------
// From this many frames on the calls are batch launches; below it they loop over the single calls (the same bits).  The rule is the one of every batch route
// here (scripts/gpu_rig_batch.py -> profiles/rig_batch_ab.txt): the smallest F from which on every batch value lies below every single-calls value on the
// lines a call stands for, 33 where no F up to 32 qualifies.  Measured, rope frames of 45 nodes under K = 3 cameras, F = 1 .. 32:
//   kRigBatchMin         lines (a) - (c): ropes that share the rig's planes from device and from pageable host planes, rigs with planes of their own.  At
//                        640 x 480 (25 429 kept pixels) the batch loses at 1 and 2 frames (a table upload and a one-workgroup finish where the single call
//                        has a team of eight: 0.137 against 0.068 ms) and wins every value from 4 on (32 ropes under one rig: 0.70 against 2.18 ms from
//                        device planes, 2.05 against 6.16 ms from host planes).  At 1280 x 720 the three cameras keep 96 805 pixels: the kernel passes every
//                        frame on, the call is its launch plus the F single calls and loses by 3 - 9 % at every F.  No F qualifies at both sizes: 33, BY
//                        DEFAULT tdlo_rig_to_cloud_batch LOOPS OVER THE SINGLE CALLS; a cell whose ropes keep fewer than 32 704 pixels sets the variable
//   kRigBatchTrackerMin  line (d), against F x tdlo_tracker_frame_from_rig: every value wins from 4 trackers on at both sizes (32 trackers: 2.26 against
//                        5.69 ms; at 1280 x 720, where the clouds take the single route, the batched pre-pass and step still win: 32.6 against 35.6 ms)
// TDLO_RIG_BATCH_MIN=n, read when the context is made, overrides both.
constexpr int kRigBatchMin = 33;
constexpr int kRigBatchTrackerMin = 4;
static int rig_batch_min(const tdlo_ctx *c, bool tracker) { return c->rig_batch_min ? c->rig_batch_min : (tracker ? kRigBatchTrackerMin : kRigBatchMin); }

int tdlo_debug_rig_batch_plan(const int *slot, const int *K, int F, int Fcap, int rows, int cols, const unsigned long long *plane, long long budget,
                              long long *state_off, long long *cams_off, long long *plane_off, long long *tiles_off, long long *pts_off, long long *cnt_off,
                              int *launch_of, long long *table_off, long long *total, int *n_planes, int *n_launches) {
    if (rows < 1 || cols < 1 || (long long)rows * cols > (1ll << 26)) return TDLO_E_INVALID;
    return rig_batch_plan(slot, K, F, Fcap, rows * cols, plane, (long long)rig_batch_desc_bytes(), (long long)sizeof(RigCam), budget > 0 ? budget : kRigBatchBudget,
                          state_off, cams_off, plane_off, tiles_off, pts_off, cnt_off, launch_of, table_off, total, n_planes, n_launches) ? TDLO_E_INVALID : TDLO_OK;
}

int tdlo_debug_rig_batch_arena(tdlo_ctx *c, const void **base, long long *bytes) {
    if (!c || !base || !bytes) return TDLO_E_INVALID;
    *base = c->rbatch_dev; *bytes = (long long)c->rbatch_dev_cap;
    return TDLO_OK;
}

static const void *rig_camera_plane(const tdlo_rig_camera &cam, bool colour, int q) {
    return q == 0 ? (const void *)cam.depth : q == 1 ? (colour ? nullptr : (const void *)cam.mask) : q == 2 ? (colour ? (const void *)cam.colour : nullptr)
                                                     : (colour ? (const void *)cam.occluder : nullptr);
}

// Everything that refuses a rig batch as a whole; nothing of the context or the slots is touched.  where[f][k]: which planes of frame f's camera k lie in device memory
static int rig_batch_refusal(tdlo_ctx *c, const tdlo_rig_frame *frames, int F, int rows, int cols, double leaf_size, std::vector<std::vector<BatchPlanes>> &where) {
    if (!frames || F < 1) return fail(c, TDLO_E_INVALID, "rig batch: no frames");
    if (F > (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "rig batch: more frames than the context has slots");
    for (int f = 0; f < F; ++f) {
        if (frames[f].slot < 0 || frames[f].slot >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
        for (int g = 0; g < f; ++g) if (frames[g].slot == frames[f].slot) return fail(c, TDLO_E_INVALID, "rig batch: a slot is named twice");
        if (const char *why = rig_fault(frames[f].cams, frames[f].K, rows, cols, leaf_size)) return fail(c, TDLO_E_INVALID, "rig batch: frame " + std::to_string(f) + ": " + why);
    }
    HIPCHK(c, hipSetDevice(c->device));
    where.assign(F, std::vector<BatchPlanes>());
    const size_t P = (size_t)rows * cols;
    for (int f = 0; f < F; ++f) {
        if (int rc = rig_refusal(c, frames[f].slot, frames[f].cams, frames[f].K, rows, cols, leaf_size, where[f])) return rc;
        const bool colour = rig_camera_colour(frames[f].cams[0]);
        for (int k = 0; k < frames[f].K; ++k)
            for (int q = 0; q < 4; ++q) {      // (a device plane is copied device to device: it must lie in neither arena a frame of this call may be served from)
                const char *p = (const char *)rig_camera_plane(frames[f].cams[k], colour, q);
                if (!p || !where[f][k].dev[q]) continue;
                const size_t len = (q == 0 ? 2 : q == 2 ? 3 : 1) * P;
                const char *a0 = (const char *)c->rbatch_dev, *b0 = (const char *)c->cbat_img;
                if ((a0 && p < a0 + c->rbatch_dev_cap && a0 < p + len) || (b0 && p < b0 + c->cbat_img_cap && b0 < p + len))
                    return fail(c, TDLO_E_INVALID, "rig batch: a device plane overlaps the batch arena");
            }
    }
    return TDLO_OK;
}

// the arena (device) and the pinned block of a rig batch, grown on demand; the state blocks armed
static int rig_batch_room(tdlo_ctx *c, size_t dev_bytes, size_t pin_bytes) {
    hipStream_t st = c->stream;
    if (dev_bytes > c->rbatch_dev_cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->rbatch_dev) hipFree(c->rbatch_dev);
        c->rbatch_dev = nullptr; c->rbatch_dev_cap = 0; c->rbatch_armed = false;
        HIPCHK(c, hipMalloc(&c->rbatch_dev, dev_bytes));
        c->rbatch_dev_cap = dev_bytes;
    }
    if (pin_bytes > c->rbatch_pin_cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->rbatch_pin) hipHostFree(c->rbatch_pin);
        c->rbatch_pin = nullptr; c->rbatch_pin_cap = 0;
        HIPCHK(c, hipHostMalloc((void **)&c->rbatch_pin, pin_bytes, hipHostMallocDefault));
        std::memset(c->rbatch_pin, 0, pin_bytes);
        c->rbatch_pin_cap = pin_bytes;
    }
    if (!c->rbatch_armed) {
        HIPCHK(c, view_batch_arm(c->rbatch_dev, (int)c->slots.size(), st));      // (the same state block: box minima ~0, everything else 0)
        c->rbatch_armed = true;
    }
    return TDLO_OK;
}

// tracker: the call stands behind the tracker entrance (rig_batch_min)
static int rig_batch_impl(tdlo_ctx *c, const tdlo_rig_frame *frames, int F, int rows, int cols, double leaf_size, int *n_out, int *n_raw_out, int *rc_each, bool tracker) {
    std::vector<std::vector<BatchPlanes>> where;
    int rc = rig_batch_refusal(c, frames, F, rows, cols, leaf_size, where);
    if (rc) return rc;
    std::vector<int> n(F, 0), nraw(F, 0), rcs(F, 0);
    auto finish = [&]() {
        if (n_out) std::copy(n.begin(), n.end(), n_out);
        if (n_raw_out) std::copy(nraw.begin(), nraw.end(), n_raw_out);
        if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
        for (int f = 0; f < F; ++f) if (rcs[f]) return rcs[f];
        return (int)TDLO_OK;
    };
    auto single = [&](int f) {
        rcs[f] = rig_to_cloud_impl(c, frames[f].slot, frames[f].cams, frames[f].K, rows, cols, leaf_size, nullptr, 0, &n[f], &nraw[f], nullptr, 0, nullptr);
    };
    if (F < rig_batch_min(c, tracker)) {
        for (int f = 0; f < F; ++f) single(f);
        return finish();
    }
    // ---- who goes into the launches, the frames that bring masks in front of the frames that bring colour: the others are passed on to the single call, after them
    const int P = rows * cols, Tc = rig_tiles_per_camera(P);
    std::vector<int> in, passed;
    for (int kind = 0; kind < 2; ++kind)
        for (int f = 0; f < F; ++f) {
            if ((rig_camera_colour(frames[f].cams[0]) ? 1 : 0) != kind) continue;
            if (c->cloud_fused_on && (long long)frames[f].K * Tc <= kRigBatchMaxTiles) in.push_back(f);
            else { passed.push_back(f); ++c->rbatch_route[1]; }
        }
    const int Fi = (int)in.size();
    if (Fi > 0) {
        hipStream_t st = c->stream;
        if (c->cloud_pending >= 0 && (rc = flush_pending_cloud(c))) return rc;
        // ---- the arena by the plan; the pinned block: result words, frame table, camera table (the two tables one behind the other, as in the arena)
        std::vector<int> slots(Fi), Ks(Fi), kinds(Fi), launch_of(Fi);
        std::vector<unsigned long long> keys;
        for (int j = 0; j < Fi; ++j) {
            const tdlo_rig_frame &fr = frames[in[j]];
            slots[j] = fr.slot; Ks[j] = fr.K; kinds[j] = rig_camera_colour(fr.cams[0]) ? 1 : 0;
            for (int k = 0; k < fr.K; ++k)
                for (int q = 0; q < 4; ++q) keys.push_back((unsigned long long)(uintptr_t)rig_camera_plane(fr.cams[k], kinds[j] != 0, q));
        }
        const size_t cams_total = keys.size() / 4;
        std::vector<long long> o_state(Fi), o_cams(Fi), o_plane(keys.size()), o_tiles(Fi), o_pts(Fi), o_cnt(Fi);
        long long o_table = 0, total = 0;
        const size_t desc = rig_batch_desc_bytes();
        if (rig_batch_plan(slots.data(), Ks.data(), Fi, (int)c->slots.size(), P, keys.data(), (long long)desc, (long long)sizeof(RigCam), kRigBatchBudget, o_state.data(),
                           o_cams.data(), o_plane.data(), o_tiles.data(), o_pts.data(), o_cnt.data(), launch_of.data(), &o_table, &total, nullptr, nullptr))
            return fail(c, TDLO_E_INVALID, "rig batch: no plan for these frames");
        auto r256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t p_tab = r256(2 * sizeof(unsigned long long) * (size_t)Fi), tab_bytes = r256(desc * (size_t)Fi), cam_bytes = sizeof(RigCam) * cams_total;
        if ((rc = rig_batch_room(c, (size_t)total, p_tab + tab_bytes + r256(cam_bytes)))) return rc;
        char *dev = (char *)c->rbatch_dev, *pin = c->rbatch_pin;
        unsigned long long *res = (unsigned long long *)pin;
        std::memset(res, 0, 2 * sizeof(unsigned long long) * (size_t)Fi);      // (no word may look like this call's epoch)
        // ---- the slots: an EMPTY slot is sized for every result the kernel can leave, as the single call sizes it; a slot with a resident cloud is launched
        // with its capacity as it is -- growing it frees the cloud, which a refused frame must find intact -- and the capacity report sends the frame on
        for (int f : in) {
            Slot &s = c->slots[frames[f].slot];
            if (s.N0 == 0 && (rc = ensure_points(c, s, cloud_fused_max_points()))) return rc;
        }
        // ---- every distinct plane once, the camera records, the descriptors
        {
            long long copied = -1;                               // (distinct planes take ascending offsets in the order of their first entries)
            size_t e = 0;
            for (int j = 0; j < Fi; ++j) {
                const tdlo_rig_frame &fr = frames[in[j]];
                for (int k = 0; k < fr.K; ++k)
                    for (int q = 0; q < 4; ++q, ++e) {
                        if (o_plane[e] < 0 || o_plane[e] <= copied) continue;
                        copied = o_plane[e];
                        const size_t len = (q == 0 ? 2 : q == 2 ? 3 : 1) * (size_t)P;
                        const hipError_t er = hipMemcpyAsync(dev + o_plane[e], (const void *)(uintptr_t)keys[e], len,
                                                             where[in[j]][k].dev[q] ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
                        if (er != hipSuccess) { (void)hipStreamSynchronize(st); HIPCHK(c, er); }
                    }
            }
        }
        RigCam *h_cam = (RigCam *)(pin + p_tab + tab_bytes);
        std::vector<RigBatchFrameHost> bf(Fi);
        {
            size_t e = 0, k0 = 0;
            for (int j = 0; j < Fi; ++j) {
                const tdlo_rig_frame &fr = frames[in[j]];
                for (int k = 0; k < fr.K; ++k, e += 4) {
                    RigCam &r = h_cam[k0 + k];
                    rig_camera_record(fr.cams[k], r);
                    r.depth = (const unsigned short *)(dev + o_plane[e]);
                    r.mask = o_plane[e + 1] >= 0 ? (const unsigned char *)(dev + o_plane[e + 1]) : nullptr;
                    r.colour = o_plane[e + 2] >= 0 ? (const unsigned char *)(dev + o_plane[e + 2]) : nullptr;
                    r.occluder = o_plane[e + 3] >= 0 ? (const unsigned char *)(dev + o_plane[e + 3]) : nullptr;
                }
                k0 += fr.K;
                Slot &s = c->slots[fr.slot];
                RigBatchFrameHost &b = bf[j];
                b = RigBatchFrameHost{};
                b.cams_dev = dev + o_cams[j]; b.K = fr.K;
                b.state = dev + o_state[j]; b.tiles = dev + o_tiles[j]; b.pts = dev + o_pts[j]; b.tcnt = dev + o_cnt[j];
                b.X = s.Xraw; b.cap = s.cap_points; b.res = res + 2 * (size_t)j;
            }
        }
        if (++c->cloud_epoch == 0) ++c->cloud_epoch;
        const unsigned epoch = c->cloud_epoch;
        const float inv = 1.0f / (float)leaf_size;
        auto enqueue = [&]() -> hipError_t {
            if (const hipError_t e = rig_batch_table(bf.data(), Fi, P, cols, inv, epoch, pin + p_tab)) return e;
            if (const hipError_t e = hipMemcpyAsync(dev + o_table, pin + p_tab, tab_bytes + cam_bytes, hipMemcpyHostToDevice, st)) return e;
            // a launch per kind and budget group, back to back: the frames [a, b) of one group and one kind stand together in the table
            for (int a = 0; a < Fi;) {
                int b = a, Tmax = 0;
                while (b < Fi && launch_of[b] == launch_of[a] && kinds[b] == kinds[a]) { Tmax = std::max(Tmax, Ks[b] * Tc); ++b; }
                if (const hipError_t e = launch_cloud_rig_batch(dev + o_table, a, b - a, Tmax, kinds[a] != 0, st)) return e;
                a = b;
            }
            return hipSuccess;
        };
        {
            hipError_t e = enqueue();
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            else (void)hipStreamSynchronize(st);                  // (whatever was enqueued has left the caller's planes and the pinned block)
            if (e != hipSuccess) { c->rbatch_armed = false; HIPCHK(c, e); }
        }
        for (int j = 0; j < Fi; ++j) {
            const int f = in[j];
            Slot &s = c->slots[frames[f].slot];
            const unsigned long long w0 = __atomic_load_n(res + 2 * (size_t)j, __ATOMIC_ACQUIRE), w1 = __atomic_load_n(res + 2 * (size_t)j + 1, __ATOMIC_RELAXED);
            const unsigned status = (unsigned)w0;
            if ((unsigned)(w0 >> 32) != epoch) { c->rbatch_armed = false; rcs[f] = fail(c, TDLO_E_HIP, "the stream drained, but a frame of the rig batch did not report"); continue; }
            nraw[f] = (int)(unsigned)(w1 >> 32);
            const int nf = (int)(unsigned)w1;
            if (status == 1u) {
                if (nf < 0 || nf > s.cap_points || nf > nraw[f]) { rcs[f] = fail(c, TDLO_E_HIP, "voxel grid produced an impossible point count"); continue; }
                n[f] = nf; s.N0 = nf; s.sorted_valid = false; ++c->rbatch_route[0];
            } else { nraw[f] = 0; passed.push_back(f); ++c->rbatch_route[1]; }      // not taken (2); the slot would have to grow (3: the single call does that)
        }
    }
    std::sort(passed.begin(), passed.end());
    for (int f : passed) single(f);
    return finish();
}

int tdlo_rig_to_cloud_batch(tdlo_ctx *c, const tdlo_rig_frame *frames, int F, int rows, int cols, double leaf_size, int *n_out, int *n_raw_out, int *rc_each) {
    if (!c) return TDLO_E_INVALID;
    return rig_batch_impl(c, frames, F, rows, cols, leaf_size, n_out, n_raw_out, rc_each, false);
}

// ---- cloud views for F slots in one call (include/trackdlo_hip.h: tdlo_cloud_view_voxel_grid_batch, tdlo_set_cloud_view_batch) --------------------------
// From this many frames on the calls are one batch launch each; below it they loop over the single calls (the same bits).  Set from
// profiles/view_batch_ab.txt and view_batch_ab_run2.txt by the rule "the smallest F from which on every batch value lies below every single-calls value", taken
// over the lines a call stands for -- TWO constants, because the data ask for it:
//   kViewBatchMin         tdlo_cloud_view_voxel_grid_batch / tdlo_set_cloud_view_batch called by themselves: the voxel lines (device and host views of 5 000
//                         points, organized 640 x 480 clouds under selections, one cloud shared by all frames) and the import lines (device, host).  ONE frame
//                         costs more as a batch on every line (0.058 against 0.041 ms for the voxel grid, 0.021 against 0.014 ms for the import: a table
//                         upload and a one-workgroup finish where the single call has a team of eight); from 2 frames on every value of every such line
//                         wins (4 device views 0.058 against 0.163 ms; 32: 0.063 against 1.29 ms, the import 0.024 against 0.43 ms)
//   kViewBatchTrackerMin  the two tracker calls: the tracker line, whose registrations bring a spread of their own, won on every value from 4 frames on in
//                         one run and from 8 in others; the largest is the constant.  (tdlo_tracker_tracking_step_view_batch has no line of its own -- not
//                         measured -- and takes the same constant.)
// TDLO_VIEW_BATCH_MIN=n, read when the context is made, overrides both.
constexpr int kViewBatchMin = 2;
constexpr int kViewBatchTrackerMin = 8;
static int view_batch_min(const tdlo_ctx *c, bool tracker) { return c->view_batch_min ? c->view_batch_min : (tracker ? kViewBatchTrackerMin : kViewBatchMin); }

int tdlo_debug_view_batch_plan(const int *N, int F, int Fcap, long long *state_off, long long *tiles_off, long long *pts_off, long long *cnt_off,
                               long long *table_off, long long *total) {
    return view_batch_plan(N, F, Fcap, (long long)view_batch_desc_bytes(), state_off, tiles_off, pts_off, cnt_off, table_off, total) ? TDLO_E_INVALID : TDLO_OK;
}

// where the views (and selection bytes) of a view batch lie
struct ViewBatchWhere { bool dev = false, sel_dev = false; };

// Everything that refuses a view batch as a whole; nothing of the context or the slots is touched.  select / leaf: the voxel grid's (select == nullptr and
// leaf_size < 0: the plain import, which has neither)
static int view_batch_refusal(tdlo_ctx *c, const char *what, const int *slots, const tdlo_cloud_view *const *views, const int *N, const unsigned char *const *select,
                              int F, bool voxel, double leaf_size, std::vector<ViewBatchWhere> &where) {
    const std::string w(what);
    if (!slots || !views || !N || F < 1) return fail(c, TDLO_E_INVALID, w + ": no frames");
    if (F > (int)c->slots.size()) return fail(c, TDLO_E_INVALID, w + ": more frames than the context has slots");
    if (voxel) {
        const float leaf = (float)leaf_size;
        if (!(leaf > 0.0f) || !std::isfinite(leaf)) return fail(c, TDLO_E_INVALID, "voxel grid: the leaf size is not a positive finite float");
    }
    for (int f = 0; f < F; ++f) {
        if (const char *why = view_fault(views[f], N[f])) return fail(c, TDLO_E_INVALID, w + ": frame " + std::to_string(f) + ": " + why);
        if (slots[f] < 0 || slots[f] >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
        for (int g = 0; g < f; ++g) if (slots[g] == slots[f]) return fail(c, TDLO_E_INVALID, w + ": a slot is named twice");
        if (views[f]->flags & TDLO_VIEW_ASYNC) return fail(c, TDLO_E_INVALID, w + ": TDLO_VIEW_ASYNC is not available (the call ends with one wait for all frames)");
        if (voxel && N[f] > (1 << 26)) return fail(c, TDLO_E_INVALID, "voxel grid on a view: more than 2^26 points");
    }
    HIPCHK(c, hipSetDevice(c->device));
    where.assign(F, ViewBatchWhere{});
    for (int f = 0; f < F; ++f) {
        if (int rc = view_location(c, views[f], &where[f].dev)) return rc;
        if (select && select[f]) { if (int rc = pointer_location(c, select[f], TDLO_MEM_AUTO, "select", &where[f].sel_dev)) return rc; }
    }
    // a device source that overlaps the resident cloud of ANY slot the call names: that cloud is written while the source is still being read
    for (int f = 0; f < F; ++f) {
        const char *a0 = nullptr, *a1 = nullptr, *b0 = nullptr, *b1 = nullptr;
        if (where[f].dev) {
            long long lo = 0, hi = 0;
            (void)tdlo_cloud_view_extent(views[f], N[f], &lo, &hi);
            a0 = (const char *)views[f]->data + lo; a1 = (const char *)views[f]->data + hi;
        }
        if (where[f].sel_dev) { b0 = (const char *)select[f]; b1 = b0 + N[f]; }
        if (!a0 && !b0) continue;
        for (int g = 0; g < F; ++g) {
            const Slot &s = c->slots[slots[g]];
            if (!s.Xraw) continue;
            const char *x0 = (const char *)s.Xraw, *x1 = x0 + 3 * (size_t)s.cap_points * sizeof(double);
            if ((a0 && a0 < x1 && x0 < a1) || (b0 && b0 < x1 && x0 < b1)) return fail(c, TDLO_E_INVALID, w + ": a view aliases the resident cloud of a slot the call names");
        }
    }
    return TDLO_OK;
}

// the arena (device) and the pinned block of a view batch, grown on demand; the state blocks armed
static int view_batch_room(tdlo_ctx *c, size_t dev_bytes, size_t pin_bytes) {
    hipStream_t st = c->stream;
    if (dev_bytes > c->wbat_dev_cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->wbat_dev) hipFree(c->wbat_dev);
        c->wbat_dev = nullptr; c->wbat_dev_cap = 0; c->wbat_armed = false;
        HIPCHK(c, hipMalloc(&c->wbat_dev, dev_bytes));
        c->wbat_dev_cap = dev_bytes;
    }
    if (pin_bytes > c->wbat_pin_cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->wbat_pin) hipHostFree(c->wbat_pin);
        c->wbat_pin = nullptr; c->wbat_pin_cap = 0;
        HIPCHK(c, hipHostMalloc((void **)&c->wbat_pin, pin_bytes, hipHostMallocDefault));
        std::memset(c->wbat_pin, 0, pin_bytes);
        c->wbat_pin_cap = pin_bytes;
    }
    if (!c->wbat_armed) {
        HIPCHK(c, view_batch_arm(c->wbat_dev, (int)c->slots.size(), st));
        c->wbat_armed = true;
    }
    return TDLO_OK;
}

// the context's stream waits for what the views' ready_streams hold so far: one event per distinct stream
static int view_batch_ready(tdlo_ctx *c, const tdlo_cloud_view *const *views, const std::vector<ViewBatchWhere> &where, const std::vector<int> &which) {
    std::vector<void *> seen;
    for (int f : which) {
        void *rs = views[f]->ready_stream;
        if (!where[f].dev || !rs || std::find(seen.begin(), seen.end(), rs) != seen.end()) continue;
        if (seen.size() >= c->wbat_ev.size()) {
            hipEvent_t e = nullptr;
            HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            c->wbat_ev.push_back(e);
        }
        hipEvent_t e = c->wbat_ev[seen.size()];
        HIPCHK(c, hipEventRecord(e, (hipStream_t)rs));
        HIPCHK(c, hipStreamWaitEvent(c->stream, e, 0));
        seen.push_back(rs);
    }
    return TDLO_OK;
}

// The host views among `which` packed column-major in their own precision behind `at` of the pinned block, every distinct view once: off[f] = where frame
// f's lies (a device view: not touched).  size_only: nothing is written, *at advances all the same.
static void view_batch_pack(const tdlo_cloud_view *const *views, const int *N, const std::vector<ViewBatchWhere> &where, const std::vector<int> &which, char *pin,
                            size_t *at, std::vector<size_t> &off, bool size_only) {
    for (size_t k = 0; k < which.size(); ++k) {
        const int f = which[k];
        if (where[f].dev) continue;
        const tdlo_cloud_view *v = views[f];
        bool had = false;
        for (size_t j = 0; j < k && !had; ++j) {
            const int g = which[j];
            const tdlo_cloud_view *u = views[g];
            if (!where[g].dev && u->data == v->data && u->dtype == v->dtype && u->stride_point == v->stride_point && u->stride_comp == v->stride_comp && N[g] == N[f]) {
                off[f] = off[g]; had = true;
            }
        }
        if (had) continue;
        const bool f64 = v->dtype == TDLO_F64;
        off[f] = *at;
        if (!size_only) {
            if (f64) view_gather((double *)(pin + *at), (const double *)v->data, v->stride_point, v->stride_comp, N[f]);
            else view_gather((float *)(pin + *at), (const float *)v->data, v->stride_point, v->stride_comp, N[f]);
        }
        *at += (3 * (size_t)N[f] * (f64 ? 8 : 4) + 255) & ~(size_t)255;
    }
}

static int view_voxel_batch_impl(tdlo_ctx *c, const int *slots, const tdlo_cloud_view *const *views, const int *N, const unsigned char *const *select, int F,
                                 double leaf_size, int *n_out, int *n_raw_out, int *rc_each, bool tracker) {
    std::vector<ViewBatchWhere> where;
    int rc = view_batch_refusal(c, "view voxel batch", slots, views, N, select, F, true, leaf_size, where);
    if (rc) return rc;
    std::vector<int> n(F, 0), nraw(F, 0), rcs(F, 0);
    auto finish = [&]() {
        if (n_out) std::copy(n.begin(), n.end(), n_out);
        if (n_raw_out) std::copy(nraw.begin(), nraw.end(), n_raw_out);
        if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
        for (int f = 0; f < F; ++f) if (rcs[f]) return rcs[f];
        return (int)TDLO_OK;
    };
    auto single = [&](int f) { rcs[f] = cloud_view_voxel_impl(c, slots[f], views[f], N[f], select[f], leaf_size, nullptr, 0, &n[f], &nraw[f], nullptr, 0, nullptr); };
    if (F < view_batch_min(c, tracker)) {
        for (int f = 0; f < F; ++f) single(f);
        return finish();
    }
    // ---- who goes into the launch: the others are passed on to the single call, after it
    std::vector<int> in, passed;
    for (int f = 0; f < F; ++f) {
        if (c->cloud_fused_on && N[f] <= view_batch_max_elements()) in.push_back(f);
        else { passed.push_back(f); ++c->wbat_route[1]; }
    }
    const int Fi = (int)in.size();
    if (Fi > 0) {
        hipStream_t st = c->stream;
        if (c->cloud_pending >= 0 && (rc = flush_pending_cloud(c))) return rc;
        // ---- the arena by the plan; the pinned block: result words, table, packed host views, host selection bytes
        std::vector<int> Ni(Fi);
        for (int j = 0; j < Fi; ++j) Ni[j] = N[in[j]];
        std::vector<long long> o_state(Fi), o_tiles(Fi), o_pts(Fi), o_cnt(Fi);
        long long o_table = 0, total = 0;
        const size_t desc = view_batch_desc_bytes();
        if (view_batch_plan(Ni.data(), Fi, (int)c->slots.size(), (long long)desc, o_state.data(), o_tiles.data(), o_pts.data(), o_cnt.data(), &o_table, &total))
            return fail(c, TDLO_E_INVALID, "view voxel batch: no plan for these frames");
        auto r256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t p_tab = r256(2 * sizeof(unsigned long long) * (size_t)Fi);
        size_t at = p_tab + r256(desc * (size_t)Fi);
        std::vector<size_t> voff(F, 0), soff(F, 0);
        const size_t p_views = at;
        view_batch_pack(views, N, where, in, nullptr, &at, voff, true);
        // (host selection bytes are READ IN PLACE from the pinned block, like the packed views: the kernel reads every byte exactly once in phase A, so a copy
        //  to the device in front of the launch would move the same bytes over the same link and add a copy command to the stream)
        for (int f : in) if (select[f] && !where[f].sel_dev) { soff[f] = at; at += r256((size_t)N[f]); }
        if ((rc = view_batch_room(c, (size_t)total, at))) return rc;
        char *dev = (char *)c->wbat_dev, *pin = c->wbat_pin;
        unsigned long long *res = (unsigned long long *)pin;
        std::memset(res, 0, 2 * sizeof(unsigned long long) * (size_t)Fi);      // (no word may look like this call's epoch)
        {
            size_t at2 = p_views;
            view_batch_pack(views, N, where, in, pin, &at2, voff, false);
        }
        for (int f : in) if (select[f] && !where[f].sel_dev) std::memcpy(pin + soff[f], select[f], (size_t)N[f]);
        // ---- the slots: room for every point the kernel can leave; whatever was resident is gone from here on
        for (int f : in) {
            Slot &s = c->slots[slots[f]];
            if ((rc = ensure_points(c, s, std::min(N[f], cloud_fused_max_points())))) return rc;
            s.N0 = 0; s.sorted_valid = false;
        }
        if ((rc = view_batch_ready(c, views, where, in))) return rc;
        std::vector<ViewBatchFrameHost> bf(Fi);
        for (int j = 0; j < Fi; ++j) {
            const int f = in[j];
            const tdlo_cloud_view *v = views[f];
            ViewBatchFrameHost &b = bf[j];
            b = ViewBatchFrameHost{};
            b.src = CloudViewSrc{v->data, v->dtype == TDLO_F64, v->stride_point, v->stride_comp, select[f]};
            if (!where[f].dev) { b.src.data = pin + voff[f]; b.src.stride_point = 1; b.src.stride_comp = N[f]; }
            if (select[f] && !where[f].sel_dev) b.src.select = (const unsigned char *)(pin + soff[f]);
            b.N = N[f];
            b.state = dev + o_state[j]; b.tiles = dev + o_tiles[j]; b.pts = dev + o_pts[j]; b.tcnt = dev + o_cnt[j];
            Slot &s = c->slots[slots[f]];
            b.X = s.Xraw; b.cap = s.cap_points; b.res = res + 2 * (size_t)j;
        }
        if (++c->cloud_epoch == 0) ++c->cloud_epoch;
        const unsigned epoch = c->cloud_epoch;
        const float inv = 1.0f / (float)leaf_size;
        {
            const hipError_t e = launch_cloud_view_batch(bf.data(), Fi, inv, epoch, pin + p_tab, dev + o_table, st);
            if (e != hipSuccess) { c->wbat_armed = false; HIPCHK(c, e); }
        }
        {
            const hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) { c->wbat_armed = false; HIPCHK(c, e); }
        }
        for (int j = 0; j < Fi; ++j) {
            const int f = in[j];
            const unsigned long long w0 = __atomic_load_n(res + 2 * (size_t)j, __ATOMIC_ACQUIRE), w1 = __atomic_load_n(res + 2 * (size_t)j + 1, __ATOMIC_RELAXED);
            const unsigned status = (unsigned)w0;
            if ((unsigned)(w0 >> 32) != epoch) { c->wbat_armed = false; rcs[f] = fail(c, TDLO_E_HIP, "the stream drained, but a frame of the view voxel batch did not report"); continue; }
            nraw[f] = (int)(unsigned)(w1 >> 32);
            const int nf = (int)(unsigned)w1;
            if (status == 1u) {
                if (nf < 0 || nf > c->slots[slots[f]].cap_points || nf > nraw[f]) { rcs[f] = fail(c, TDLO_E_HIP, "voxel grid produced an impossible point count"); continue; }
                n[f] = nf; c->slots[slots[f]].N0 = nf; ++c->wbat_route[0];
            } else { passed.push_back(f); ++c->wbat_route[1]; }      // not taken (2); the slot would have to grow (3: the single call does that)
        }
    }
    std::sort(passed.begin(), passed.end());
    for (int f : passed) single(f);
    return finish();
}

// tracker: the call stands behind a tracker entrance (view_batch_min)
static int view_voxel_batch_frames(tdlo_ctx *c, const tdlo_view_frame *frames, int F, double leaf_size, int *n_out, int *n_raw_out, int *rc_each, bool tracker) {
    if (!frames || F < 1) return fail(c, TDLO_E_INVALID, "view voxel batch: no frames");
    std::vector<int> slots(F), N(F);
    std::vector<const tdlo_cloud_view *> views(F);
    std::vector<const unsigned char *> sel(F);
    for (int f = 0; f < F; ++f) { slots[f] = frames[f].slot; views[f] = frames[f].view; N[f] = frames[f].N; sel[f] = frames[f].select; }
    return view_voxel_batch_impl(c, slots.data(), views.data(), N.data(), sel.data(), F, leaf_size, n_out, n_raw_out, rc_each, tracker);
}

int tdlo_cloud_view_voxel_grid_batch(tdlo_ctx *c, const tdlo_view_frame *frames, int F, double leaf_size, int *n_out, int *n_raw_out, int *rc_each) {
    if (!c) return TDLO_E_INVALID;
    return view_voxel_batch_frames(c, frames, F, leaf_size, n_out, n_raw_out, rc_each, false);
}

// tdlo_set_cloud_view_batch on checked arguments.  wait: the call returns when the imports have finished (false: the tracker call, whose registrations wait
// for the stream before it returns -- the pinned block is free again by then)
static int view_import_batch_impl(tdlo_ctx *c, const int *slots, const tdlo_cloud_view *const *views, const int *N, int F, int *rc_each, bool wait, bool tracker) {
    std::vector<ViewBatchWhere> where;
    int rc = view_batch_refusal(c, "view import batch", slots, views, N, nullptr, F, false, -1.0, where);
    if (rc) return rc;
    std::vector<int> rcs(F, 0);
    auto finish = [&]() {
        if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
        for (int f = 0; f < F; ++f) if (rcs[f]) return rcs[f];
        return (int)TDLO_OK;
    };
    if (F < view_batch_min(c, tracker)) {
        for (int f = 0; f < F; ++f) { rcs[f] = import_view(c, slots[f], views[f], N[f], where[f].dev, wait || !where[f].dev); if (!rcs[f]) ++c->wbat_route[3]; }
        return finish();
    }
    hipStream_t st = c->stream;
    if ((rc = flush_pending_cloud(c))) return rc;
    std::vector<int> all(F);
    for (int f = 0; f < F; ++f) all[f] = f;
    auto r256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t tab = r256(sizeof(ImportBatchFrame) * (size_t)F);
    std::vector<size_t> voff(F, 0);
    size_t at = tab;
    view_batch_pack(views, N, where, all, nullptr, &at, voff, true);
    const size_t packed = at - tab;
    // the arena: [state blocks (the voxel grid's: not touched) | table | TDLO_VIEW_INPLACE=0: the packed views' copy]
    const size_t d_tab = (size_t)kViewBatchState * c->slots.size();
    if ((rc = view_batch_room(c, d_tab + tab + (c->view_inplace ? 0 : packed), at))) return rc;
    char *dev = (char *)c->wbat_dev, *pin = c->wbat_pin;
    {
        size_t at2 = tab;
        view_batch_pack(views, N, where, all, pin, &at2, voff, false);
    }
    for (int f = 0; f < F; ++f) if ((rc = ensure_points(c, c->slots[slots[f]], N[f]))) return rc;
    if ((rc = view_batch_ready(c, views, where, all))) return rc;
    if (!c->view_inplace && packed > 0) HIPCHK(c, hipMemcpyAsync(dev + d_tab + tab, pin + tab, packed, hipMemcpyHostToDevice, st));
    std::vector<ImportBatchFrame> bf(F);
    std::vector<char> f64(F);
    for (int f = 0; f < F; ++f) {
        const tdlo_cloud_view *v = views[f];
        f64[f] = v->dtype == TDLO_F64;
        if (where[f].dev) bf[f] = ImportBatchFrame{v->data, v->stride_point, v->stride_comp, c->slots[slots[f]].Xraw, N[f], 0};
        else bf[f] = ImportBatchFrame{(c->view_inplace ? pin : dev + d_tab) + voff[f], 1, (long long)N[f], c->slots[slots[f]].Xraw, N[f], 0};
    }
    HIPCHK(c, launch_cloud_import_batch(bf.data(), (const bool *)f64.data(), F, pin, dev + d_tab, st));
    for (int f = 0; f < F; ++f) { Slot &s = c->slots[slots[f]]; s.N0 = N[f]; s.sorted_valid = false; }
    c->wbat_route[2] += F;
    if (wait) HIPCHK(c, wait_stream(st));
    return finish();
}

int tdlo_set_cloud_view_batch(tdlo_ctx *c, const int *slots, const tdlo_cloud_view *const *views, const int *N, int F, int *rc_each) {
    if (!c) return TDLO_E_INVALID;
    return view_import_batch_impl(c, slots, views, N, F, rc_each, true, false);
}

// ---- caller-side visibility pre-pass ------------------------------------------------------------
static void vis_threshold_and_fill(const double *min_d2, int M, double visibility_threshold, double d_vis, const double *geodesic_coord, double *node_dist,
                                   int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext);

int tdlo_visibility_prepass(tdlo_ctx *c, int slot, const double *Y, int M, double visibility_threshold, double d_vis,
                            const double *geodesic_coord, double *node_dist, int *visible_nodes, int *n_vis,
                            int *visible_nodes_extended, int *n_vis_ext) {
    if (!c) return TDLO_E_INVALID;
    if (slot < 0 || slot >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
    if (!Y || M < 1 || !geodesic_coord) return fail(c, TDLO_E_INVALID, "null Y / geodesic_coord");
    Slot &s = c->slots[slot];
    if (s.N0 <= 0) return fail(c, TDLO_E_INVALID, "no cloud resident in slot (call tdlo_set_cloud)");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_nodes(c, s, M);
    if (rc) return rc;
    rc = ensure_pin(c, 4 * (size_t)M + 8);
    if (rc) return rc;
    NodeCarve nc(M);
    hipStream_t st = c->stream;
    if (c->cloud_pending >= 0 && (rc = flush_pending_cloud(c))) return rc;
    std::memcpy(c->pin, Y, sizeof(double) * 3 * M);
    if (c->direct_in && M <= kMaxNodes) {
        // one launch, no copies: the kernel reads the nodes from the pinned staging block and its last workgroup writes the minima to pinned host
        // memory (TDLO_DIRECT_UPLOAD=0: the copies + stream synchronisation below, the comparator)
        if ((rc = ensure_vis_state(c))) return rc;
        if (++c->vis_epoch == 0) ++c->vis_epoch;
        ++c->vis_route[0];
        HIPCHK(c, launch_node_min_dist_direct(s.Xraw, s.N0, c->pin, M, c->vis_state, c->vis_res, c->vis_epoch, st));
        auto t_chk = std::chrono::steady_clock::now();
        for (unsigned spins = 1;; ++spins) {
            if ((unsigned)__atomic_load_n(c->vis_res, __ATOMIC_ACQUIRE) == c->vis_epoch) break;
            if ((spins & 255u) == 0) {
                const auto now = std::chrono::steady_clock::now();
                if (std::chrono::duration<double, std::micro>(now - t_chk).count() > 500.0) {
                    t_chk = now;
                    const hipError_t e = hipStreamQuery(st);
                    if (e == hipSuccess) {
                        if ((unsigned)__atomic_load_n(c->vis_res, __ATOMIC_ACQUIRE) == c->vis_epoch) break;
                        c->vis_armed = false;
                        return fail(c, TDLO_E_HIP, "the stream drained, but the visibility pre-pass did not report");
                    }
                    if (e != hipErrorNotReady) { c->vis_armed = false; return fail(c, TDLO_E_HIP, std::string("stream: ") + hipGetErrorString(e)); }
                }
            }
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        }
        std::memcpy(c->pin, c->vis_res + 1, sizeof(double) * M);
    } else {
        double *dY = s.nodeblk + nc.Yin;                                  // reuse the node upload area
        unsigned long long *dbits = (unsigned long long *)(s.nodeblk + nc.dmin);
        for (int m = 0; m < M; ++m) { const unsigned long long inf = 0x7ff0000000000000ull; std::memcpy(c->pin + 3 * M + m, &inf, 8); }
        HIPCHK(c, hipMemcpyAsync(dY, c->pin, sizeof(double) * 3 * M, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(dbits, c->pin + 3 * M, sizeof(double) * M, hipMemcpyHostToDevice, st));
        ++c->vis_route[1];
        HIPCHK(c, launch_node_min_dist(s.Xraw, s.N0, dY, M, dbits, st));
        HIPCHK(c, hipMemcpyAsync(c->pin, dbits, sizeof(double) * M, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    vis_threshold_and_fill(c->pin, M, visibility_threshold, d_vis, geodesic_coord, node_dist, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext);
    return TDLO_OK;      // an empty visible set is reported as n_vis = 0 (the reference underflows at :351)
}

// the batch's own state for F M minima: replaced by a larger one (the stream drained first), armed when allocated or after a launch that did not report
static int ensure_vbat_state(tdlo_ctx *c, size_t FM) {
    if (FM > c->vbat_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->vbat_state) hipFree(c->vbat_state);
        if (c->vbat_res) hipHostFree(c->vbat_res);
        c->vbat_state = nullptr; c->vbat_res = nullptr; c->vbat_cap = 0;
        const size_t cap = (FM + 1023) & ~(size_t)1023;
        HIPCHK(c, hipMalloc((void **)&c->vbat_state, sizeof(unsigned long long) * (cap + 8)));
        HIPCHK(c, hipHostMalloc((void **)&c->vbat_res, sizeof(unsigned long long) * (cap + 8), hipHostMallocDefault));
        std::memset(c->vbat_res, 0, sizeof(unsigned long long) * (cap + 8));
        c->vbat_cap = cap; c->vbat_armed = false; c->vbat_epoch = 0;
    }
    if (!c->vbat_armed) {
        std::vector<unsigned long long> init(c->vbat_cap + 8, 0x7ff0000000000000ull);
        for (size_t i = c->vbat_cap; i < c->vbat_cap + 8; ++i) init[i] = 0ull;
        HIPCHK(c, hipMemcpy(c->vbat_state, init.data(), sizeof(unsigned long long) * init.size(), hipMemcpyHostToDevice));
        c->vbat_armed = true;
    }
    return TDLO_OK;
}

// tdlo_visibility_prepass for F slots: ONE launch and one wait (k_node_min_dist_batch), then the thresholding and gap fill per frame.  Where the single call
// does not take its one-launch kernel (TDLO_DIRECT_UPLOAD=0, M > 1024), and for one slot, the call loops over it.  The bits are the single call's on every route.
int tdlo_visibility_prepass_batch(tdlo_ctx *c, int F, const int *slots, const double *Y, int M, double visibility_threshold, double d_vis,
                                  const double *geodesic_coord, double *node_dist, int *visible_nodes, int *n_vis,
                                  int *visible_nodes_extended, int *n_vis_ext) {
    if (!c) return TDLO_E_INVALID;
    if (F < 1 || F > (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad frame count");
    if (!slots || !Y || M < 1 || !geodesic_coord) return fail(c, TDLO_E_INVALID, "null slots / Y / geodesic_coord");
    for (int i = 0; i < F; ++i) {
        if (slots[i] < 0 || slots[i] >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
        for (int j = 0; j < i; ++j) if (slots[j] == slots[i]) return fail(c, TDLO_E_INVALID, "the slots of a batch must be distinct");
        if (c->slots[slots[i]].N0 <= 0) return fail(c, TDLO_E_INVALID, "no cloud resident in slot (call tdlo_set_cloud)");
    }
    auto at = [&](auto *p, int i) { return p ? p + (size_t)i * M : nullptr; };
    auto at1 = [&](int *p, int i) { return p ? p + i : nullptr; };
    if (F == 1 || !c->direct_in || M > kMaxNodes) {      // (one slot: the single call's kernel has no frame table to fetch first -- 0.035 against 0.044 ms for one slot, profiles/tracker_batch_ab.txt)
        ++c->vbat_route[1];
        for (int i = 0; i < F; ++i) {
            const int rc = tdlo_visibility_prepass(c, slots[i], Y + (size_t)i * 3 * M, M, visibility_threshold, d_vis, geodesic_coord + (size_t)i * M, at(node_dist, i),
                                                   at(visible_nodes, i), at1(n_vis, i), at(visible_nodes_extended, i), at1(n_vis_ext, i));
            if (rc) return rc;
        }
        return TDLO_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t FM = (size_t)F * M;
    // the pinned staging block: [VisBatchFrame x F | wg0 x (F + 1) | F node blocks]
    const size_t tab_doubles = ((size_t)F * sizeof(VisBatchFrame) + 7) / 8, wg_doubles = ((size_t)(F + 1) * sizeof(int) + 7) / 8;
    if ((rc = ensure_pin(c, tab_doubles + wg_doubles + 3 * FM + 8))) return rc;
    if (c->cloud_pending >= 0 && (rc = flush_pending_cloud(c))) return rc;
    if ((rc = ensure_vbat_state(c, FM))) return rc;
    VisBatchFrame *tab = (VisBatchFrame *)c->pin;
    int *wg0 = (int *)(c->pin + tab_doubles);
    double *Yp = c->pin + tab_doubles + wg_doubles;
    int nwg = 0;
    for (int i = 0; i < F; ++i) {
        const Slot &s = c->slots[slots[i]];
        tab[i].X = s.Xraw; tab[i].N0 = s.N0; tab[i].pad = 0;
        wg0[i] = nwg;
        nwg += node_min_dist_batch_wgs(s.N0);
    }
    wg0[F] = nwg;
    std::memcpy(Yp, Y, sizeof(double) * 3 * FM);
    hipStream_t st = c->stream;
    if (++c->vbat_epoch == 0) ++c->vbat_epoch;
    ++c->vbat_route[0];
    HIPCHK(c, launch_node_min_dist_batch(tab, wg0, Yp, F, M, nwg, c->vbat_state, c->vbat_state + c->vbat_cap, c->vbat_res, c->vbat_epoch, st));
    auto t_chk = std::chrono::steady_clock::now();
    for (unsigned spins = 1;; ++spins) {
        if ((unsigned)__atomic_load_n(c->vbat_res, __ATOMIC_ACQUIRE) == c->vbat_epoch) break;
        if ((spins & 255u) == 0) {
            const auto now = std::chrono::steady_clock::now();
            if (std::chrono::duration<double, std::micro>(now - t_chk).count() > 500.0) {
                t_chk = now;
                const hipError_t e = hipStreamQuery(st);
                if (e == hipSuccess) {
                    if ((unsigned)__atomic_load_n(c->vbat_res, __ATOMIC_ACQUIRE) == c->vbat_epoch) break;
                    c->vbat_armed = false;
                    return fail(c, TDLO_E_HIP, "the stream drained, but the batched visibility pre-pass did not report");
                }
                if (e != hipErrorNotReady) { c->vbat_armed = false; return fail(c, TDLO_E_HIP, std::string("stream: ") + hipGetErrorString(e)); }
            }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    const double *mins = (const double *)(c->vbat_res + 1);
    for (int i = 0; i < F; ++i)
        vis_threshold_and_fill(mins + (size_t)i * M, M, visibility_threshold, d_vis, geodesic_coord + (size_t)i * M, at(node_dist, i), at(visible_nodes, i), at1(n_vis, i),
                               at(visible_nodes_extended, i), at1(n_vis_ext, i));
    return TDLO_OK;
}

// trackdlo_node.cpp:348-360: occluded runs shorter than d_vis (in the geodesic coordinate) between two visible nodes are filled in
static void fill_visible_gaps(const std::vector<int> &vis, const double *geodesic_coord, double d_vis, std::vector<int> &ext) {
    ext.clear();
    if (vis.empty()) return;
    for (size_t i = 0; i + 1 < vis.size(); ++i) {
        ext.push_back(vis[i]);
        if (std::fabs(geodesic_coord[vis[i + 1]] - geodesic_coord[vis[i]]) <= d_vis)
            for (int j = 1; j < vis[i + 1] - vis[i]; ++j) ext.push_back(vis[i] + j);
    }
    ext.push_back(vis.back());
}

// thresholding and gap fill on the host (O(M)) from the squared minima: trackdlo_node.cpp:316/:326 (distance test only; the painter test of
// :279-343 is tdlo_self_occlusion_visible, applied by the caller or by a tracker it was switched on for), :345-360
static void vis_threshold_and_fill(const double *min_d2, int M, double visibility_threshold, double d_vis, const double *geodesic_coord, double *node_dist,
                                   int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext) {
    std::vector<int> vis;
    for (int m = 0; m < M; ++m) {
        const double d = std::min(std::sqrt(min_d2[m]), 100000.0);       // :261: the reference's search starts from 100000 (a cloud without a finite point)
        if (node_dist) node_dist[m] = d;
        if (d <= visibility_threshold) vis.push_back(m);
    }
    if (n_vis) *n_vis = (int)vis.size();
    if (visible_nodes) std::copy(vis.begin(), vis.end(), visible_nodes);
    std::vector<int> ext;
    fill_visible_gaps(vis, geodesic_coord, d_vis, ext);
    if (n_vis_ext) *n_vis_ext = (int)ext.size();
    if (visible_nodes_extended) std::copy(ext.begin(), ext.end(), visible_nodes_extended);
}

// One frame of the ROS node up to tracking_step (trackdlo_node.cpp:195-277, :345-360) in one call: depth image -> cloud -> voxel grid, and the visibility
// pre-pass of the tracker's current nodes against that cloud.  With up to 64 nodes and the one-launch team kernel the pre-pass rides in the same launch
// (every team member takes the minima over the centroids it has just formed): one launch and one hand-over through pinned memory for both steps.
// Otherwise -- more nodes, TDLO_CLOUD_TEAM=0, too many masked pixels, a team that gave up -- tdlo_visibility_prepass runs behind it: the same numbers.
static int depth_to_cloud_visibility_impl(tdlo_ctx *c, int slot, const unsigned short *depth, const unsigned char *mask, const ColourIn *colour, int rows, int cols,
                                          double fx, double fy, double cx, double cy, double leaf_size,
                                          const double *Y, int M, double visibility_threshold, double d_vis, const double *geodesic_coord,
                                          double *node_dist, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                          int *n_out, int *n_raw_out) {
    if (!c) return TDLO_E_INVALID;
    if (!Y || M < 1 || !geodesic_coord) return fail(c, TDLO_E_INVALID, "null Y / geodesic_coord");
    bool vis_done = false;
    int n = 0;
    int rc = depth_to_cloud_impl(c, slot, depth, mask, rows, cols, fx, fy, cx, cy, leaf_size, nullptr, 0, &n, n_raw_out, Y, M, &vis_done, colour);
    if (n_out) *n_out = n;
    if (rc) return rc;
    if (n_vis) *n_vis = 0;
    if (n_vis_ext) *n_vis_ext = 0;
    if (n == 0) return TDLO_OK;                  // no cloud, nothing visible (tdlo_visibility_prepass would refuse the empty slot)
    if (!vis_done) return tdlo_visibility_prepass(c, slot, Y, M, visibility_threshold, d_vis, geodesic_coord, node_dist, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext);
    if ((rc = ensure_pin(c, (size_t)M + 8))) return rc;
    std::memcpy(c->pin, c->vis_res + 1, sizeof(double) * M);
    vis_threshold_and_fill(c->pin, M, visibility_threshold, d_vis, geodesic_coord, node_dist, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext);
    return TDLO_OK;
}

// The view counterpart: V(view, N, select, leaf) into the slot and the pre-pass against it; with up to 64 nodes it rides in the team kernel's launch
int tdlo_cloud_view_voxel_grid_visibility(tdlo_ctx *c, int slot, const tdlo_cloud_view *v, int N, const unsigned char *select, double leaf_size,
                                          const double *Y, int M, double visibility_threshold, double d_vis, const double *geodesic_coord,
                                          double *node_dist, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                          int *n_out, int *n_raw_out) {
    if (!c) return TDLO_E_INVALID;
    if (!Y || M < 1 || !geodesic_coord) return fail(c, TDLO_E_INVALID, "null Y / geodesic_coord");
    bool vis_done = false;
    int n = 0;
    int rc = cloud_view_voxel_impl(c, slot, v, N, select, leaf_size, nullptr, 0, &n, n_raw_out, Y, M, &vis_done);
    if (n_out) *n_out = n;
    if (rc) return rc;
    if (n_vis) *n_vis = 0;
    if (n_vis_ext) *n_vis_ext = 0;
    if (n == 0) return TDLO_OK;                  // no cloud, nothing visible (tdlo_visibility_prepass would refuse the empty slot)
    if (!vis_done) return tdlo_visibility_prepass(c, slot, Y, M, visibility_threshold, d_vis, geodesic_coord, node_dist, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext);
    if ((rc = ensure_pin(c, (size_t)M + 8))) return rc;
    std::memcpy(c->pin, c->vis_res + 1, sizeof(double) * M);
    vis_threshold_and_fill(c->pin, M, visibility_threshold, d_vis, geodesic_coord, node_dist, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext);
    return TDLO_OK;
}

// The rig counterpart: V(R, leaf) into the slot and the pre-pass against it; with up to 64 nodes it rides in the team kernel's launch
int tdlo_rig_to_cloud_visibility(tdlo_ctx *c, int slot, const tdlo_rig_camera *cams, int K, int rows, int cols, double leaf_size,
                                 const double *Y, int M, double visibility_threshold, double d_vis, const double *geodesic_coord,
                                 double *node_dist, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                 int *n_out, int *n_raw_out) {
    if (!c) return TDLO_E_INVALID;
    if (!Y || M < 1 || !geodesic_coord) return fail(c, TDLO_E_INVALID, "null Y / geodesic_coord");
    bool vis_done = false;
    int n = 0;
    int rc = rig_to_cloud_impl(c, slot, cams, K, rows, cols, leaf_size, nullptr, 0, &n, n_raw_out, Y, M, &vis_done);
    if (n_out) *n_out = n;
    if (rc) return rc;
    if (n_vis) *n_vis = 0;
    if (n_vis_ext) *n_vis_ext = 0;
    if (n == 0) return TDLO_OK;                  // no cloud, nothing visible (tdlo_visibility_prepass would refuse the empty slot)
    if (!vis_done) return tdlo_visibility_prepass(c, slot, Y, M, visibility_threshold, d_vis, geodesic_coord, node_dist, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext);
    if ((rc = ensure_pin(c, (size_t)M + 8))) return rc;
    std::memcpy(c->pin, c->vis_res + 1, sizeof(double) * M);
    vis_threshold_and_fill(c->pin, M, visibility_threshold, d_vis, geodesic_coord, node_dist, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext);
    return TDLO_OK;
}

int tdlo_depth_to_cloud_visibility(tdlo_ctx *c, int slot, const unsigned short *depth, const unsigned char *mask, int rows, int cols,
                                   double fx, double fy, double cx, double cy, double leaf_size,
                                   const double *Y, int M, double visibility_threshold, double d_vis, const double *geodesic_coord,
                                   double *node_dist, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                   int *n_out, int *n_raw_out) {
    return depth_to_cloud_visibility_impl(c, slot, depth, mask, nullptr, rows, cols, fx, fy, cx, cy, leaf_size, Y, M, visibility_threshold, d_vis, geodesic_coord,
                                          node_dist, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext, n_out, n_raw_out);
}

int tdlo_colour_depth_to_cloud_visibility(tdlo_ctx *c, int slot, const unsigned short *depth, const unsigned char *colour, const tdlo_colour_params *params,
                                          const unsigned char *occluder, int rows, int cols, double fx, double fy, double cx, double cy, double leaf_size,
                                          const double *Y, int M, double visibility_threshold, double d_vis, const double *geodesic_coord,
                                          double *node_dist, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                          int *n_out, int *n_raw_out) {
    const ColourIn ci{colour, params, occluder};
    return depth_to_cloud_visibility_impl(c, slot, depth, nullptr, &ci, rows, cols, fx, fy, cx, cy, leaf_size, Y, M, visibility_threshold, d_vis, geodesic_coord,
                                          node_dist, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext, n_out, n_raw_out);
}

// ---- frames as they arrive: image views in device or host memory (tdlo_image_view; tdlo_image.h) ---------------------------------------------
// The canonical images of a checked frame view, where the packed routes read them without a copy of their own.
struct StagedFrame { const unsigned short *depth = nullptr; const unsigned char *mask = nullptr; ColourIn ci{nullptr, nullptr, nullptr}; bool colour = false; };

// nullptr: fv describes a frame of rows x cols images; otherwise what is wrong with it
static const char *frame_view_fault(const tdlo_frame_view *fv, int rows, int cols) {
    if (!fv) return "frame view: null";
    if (!fv->depth.data) return "frame view: no depth image";
    if ((fv->mask.data != nullptr) == (fv->colour.data != nullptr)) return "frame view: exactly one of mask and colour";
    if (fv->mask.data && fv->occluder.data) return "frame view: an occluder goes with a colour image, not with a mask";
    const tdlo_image_view *iv[4] = {&fv->depth, &fv->colour, &fv->occluder, &fv->mask};
    for (int r = 0; r < 4; ++r)
        if (iv[r]->data)
            if (const char *why = image_view_fault(iv[r], rows, cols, r)) return why;
    return nullptr;
}

// Everything a view call refuses before it touches the context: the frame, the colour parameters, the slot, the leaf and the intrinsics
static int frame_view_refusal(tdlo_ctx *c, int slot, const tdlo_frame_view *fv, const tdlo_colour_params *cp, int rows, int cols, double fx, double fy, double leaf_size) {
    if (const char *why = frame_view_fault(fv, rows, cols)) return fail(c, TDLO_E_INVALID, why);
    CloudColour cc;
    if (fv->colour.data && !colour_pack(cp, cc)) return fail(c, TDLO_E_INVALID, "tdlo_colour_params: 1 .. 4 ranges");
    if (slot < 0 || slot >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
    if (!(leaf_size > 0) || fx == 0 || fy == 0) return fail(c, TDLO_E_INVALID, "bad leaf size / intrinsics");
    return TDLO_OK;
}

// Where a checked image view lies (pointer_location), and the one thing a host view must not do
static int image_view_where(tdlo_ctx *c, const tdlo_image_view *v, int rows, int cols, bool *device) {
    if (int rc = pointer_location(c, v->data, v->location, "image view", device)) return rc;
    if (*device) return TDLO_OK;
    long long lo, hi;
    image_view_span(v, rows, cols, &lo, &hi);
    const char *a = (const char *)v->data + lo, *b = (const char *)v->data + hi;
    if ((c->img_pin && a < c->img_pin + c->img_pin_cap && b > c->img_pin) || (c->col_pin && a < c->col_pin + c->col_pin_cap && b > c->col_pin))
        return fail(c, TDLO_E_INVALID, "image view: a host view inside the context's pinned image buffers (hand those to the packed calls)");
    return TDLO_OK;
}

// A checked frame view -> its canonical images.  Device sources: one launch of k_image_import into the device image buffers (cloud_ws: depth | mask,
// col_dev: colour | occluder), which depth_to_cloud_impl / colour_stage recognise by their addresses.  Host sources: packed and converted by the host
// into the pinned buffers of tdlo_image_buffers / tdlo_colour_buffers, i.e. the in-place route; in a frame that has device sources too they are
// copied on to the device buffers.
static int stage_frame_view(tdlo_ctx *c, const tdlo_frame_view *fv, const tdlo_colour_params *cp, int rows, int cols, StagedFrame &sf) {
    HIPCHK(c, hipSetDevice(c->device));
    const size_t P = (size_t)rows * cols;
    const tdlo_image_view *iv[4] = {&fv->depth, &fv->colour, &fv->occluder, &fv->mask};
    const size_t bytes[4] = {2 * P, 3 * P, P, P};
    bool dev[4] = {false, false, false, false}, any_dev = false, any_host = false;
    for (int r = 0; r < 4; ++r) {
        if (!iv[r]->data) continue;
        if (int rc = image_view_where(c, iv[r], rows, cols, &dev[r])) return rc;
        if (dev[r]) any_dev = true; else any_host = true;
    }
    sf.colour = fv->colour.data != nullptr;
    const bool want_col = sf.colour;
    unsigned char *pin[4] = {nullptr, nullptr, nullptr, nullptr}, *dst[4] = {nullptr, nullptr, nullptr, nullptr};
    if (any_host) {
        unsigned short *pd = nullptr;
        if (int rc = tdlo_image_buffers(c, rows, cols, &pd, &pin[kRoleMask])) return rc;
        pin[kRoleDepth] = (unsigned char *)pd;
        if (want_col)
            if (int rc = tdlo_colour_buffers(c, rows, cols, &pin[kRoleColour], &pin[kRoleOccluder])) return rc;
        for (int r = 0; r < 4; ++r)
            if (iv[r]->data && !dev[r]) image_pack_host(iv[r], rows, cols, pin[r]);
    }
    if (any_dev) {
        if (int rc = ensure_cloud_ws(c, (int)P)) return rc;
        dst[kRoleDepth] = (unsigned char *)c->cloud_ws;
        dst[kRoleMask] = (unsigned char *)c->cloud_ws + img_depth_bytes(P);
        if (want_col) {
            const size_t need = img_colour_bytes(P) + img_occ_bytes(P);
            if (need > c->col_dev_cap) {
                HIPCHK(c, hipStreamSynchronize(c->stream));
                if (c->col_dev) hipFree(c->col_dev);
                c->col_dev = nullptr; c->col_dev_cap = 0; c->last_colour = c->last_occluder = nullptr;
                HIPCHK(c, hipMalloc(&c->col_dev, need));
                c->col_dev_cap = need;
            }
            dst[kRoleColour] = (unsigned char *)c->col_dev;
            dst[kRoleOccluder] = (unsigned char *)c->col_dev + img_colour_bytes(P);
        }
        ImageJob job{};
        job.P = (int)P; job.cols = cols;
        for (int r = 0; r < 4; ++r) {
            if (!iv[r]->data) continue;
            if (!dev[r]) { HIPCHK(c, hipMemcpyAsync(dst[r], pin[r], bytes[r], hipMemcpyHostToDevice, c->stream)); continue; }
            if (iv[r]->ready_stream) {
                if (!c->ev_view) HIPCHK(c, hipEventCreateWithFlags(&c->ev_view, hipEventDisableTiming));
                HIPCHK(c, hipEventRecord(c->ev_view, (hipStream_t)iv[r]->ready_stream));
                HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_view, 0));
            }
            job.src[r] = ImageSrc{(const unsigned char *)iv[r]->data, iv[r]->row_stride, iv[r]->format, image_import_form(iv[r]->data, iv[r]->row_stride, cols, iv[r]->format)};
            job.dst[r] = dst[r];
        }
        HIPCHK(c, launch_image_import(job, c->stream));
    }
    unsigned char **where = any_dev ? dst : pin;
    for (int r = 0; r < 4; ++r) c->view_img[r] = iv[r]->data ? where[r] : nullptr;
    c->view_rows = rows; c->view_cols = cols;
    sf.depth = (const unsigned short *)where[kRoleDepth];
    sf.mask = fv->mask.data ? where[kRoleMask] : nullptr;
    sf.ci = ColourIn{want_col ? where[kRoleColour] : nullptr, cp, fv->occluder.data ? where[kRoleOccluder] : nullptr};
    return TDLO_OK;
}

int tdlo_frame_to_cloud_view(tdlo_ctx *c, int slot, const tdlo_frame_view *fv, const tdlo_colour_params *colour_params, int rows, int cols,
                             double fx, double fy, double cx, double cy, double leaf_size, double *X_out, int x_capacity, int *n_out, int *n_raw_out) {
    if (!c) return TDLO_E_INVALID;
    int rc = frame_view_refusal(c, slot, fv, colour_params, rows, cols, fx, fy, leaf_size);
    if (rc) return rc;
    StagedFrame sf;
    if ((rc = stage_frame_view(c, fv, colour_params, rows, cols, sf))) return rc;
    return depth_to_cloud_impl(c, slot, sf.depth, sf.mask, rows, cols, fx, fy, cx, cy, leaf_size, X_out, x_capacity, n_out, n_raw_out, nullptr, 0, nullptr,
                               sf.colour ? &sf.ci : nullptr);
}

int tdlo_frame_to_cloud_visibility_view(tdlo_ctx *c, int slot, const tdlo_frame_view *fv, const tdlo_colour_params *colour_params, int rows, int cols,
                                        double fx, double fy, double cx, double cy, double leaf_size,
                                        const double *Y, int M, double visibility_threshold, double d_vis, const double *geodesic_coord,
                                        double *node_dist, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                        int *n_out, int *n_raw_out) {
    if (!c) return TDLO_E_INVALID;
    if (!Y || M < 1 || !geodesic_coord) return fail(c, TDLO_E_INVALID, "null Y / geodesic_coord");
    int rc = frame_view_refusal(c, slot, fv, colour_params, rows, cols, fx, fy, leaf_size);
    if (rc) return rc;
    StagedFrame sf;
    if ((rc = stage_frame_view(c, fv, colour_params, rows, cols, sf))) return rc;
    return depth_to_cloud_visibility_impl(c, slot, sf.depth, sf.mask, sf.colour ? &sf.ci : nullptr, rows, cols, fx, fy, cx, cy, leaf_size, Y, M, visibility_threshold,
                                          d_vis, geodesic_coord, node_dist, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext, n_out, n_raw_out);
}

// ---- depth aligned to the colour camera (include/trackdlo_hip.h: tdlo_align_depth; tdlo_align.hip, tdlo_align_host.cpp) ------------------------------------
// aln_dev = [4 count words (256 bytes) | scratch: cap_c words | aligned plane: cap_c uint16 | packed depth of a host view: cap_d uint16], every block 256-byte
// aligned; aln_pin = [packed depth: cap_d uint16 | the host route's plane: cap_c uint16].  Grown together when either camera's size passes its capacity.
static size_t aln_round(size_t b) { return (b + 255) & ~(size_t)255; }
static unsigned long long *aln_counts(tdlo_ctx *c) { return (unsigned long long *)c->aln_dev; }
static unsigned *aln_scratch(tdlo_ctx *c) { return (unsigned *)(c->aln_dev + 256); }
static unsigned short *aln_plane(tdlo_ctx *c) { return (unsigned short *)(c->aln_dev + 256 + aln_round(4 * c->aln_Pc)); }
static unsigned short *aln_depth(tdlo_ctx *c) { return (unsigned short *)(c->aln_dev + 256 + aln_round(4 * c->aln_Pc) + aln_round(2 * c->aln_Pc)); }
static unsigned short *aln_pin_plane(tdlo_ctx *c) { return (unsigned short *)(c->aln_pin + aln_round(2 * c->aln_Pd)); }

static int align_reserve(tdlo_ctx *c, size_t Pc, size_t Pd) {
    if (!c->aln_res) {
        HIPCHK(c, hipHostMalloc((void **)&c->aln_res, 8 * sizeof(unsigned long long), hipHostMallocDefault));
        std::memset(c->aln_res, 0, 8 * sizeof(unsigned long long));
    }
    if (Pc <= c->aln_Pc && Pd <= c->aln_Pd && c->aln_dev && c->aln_pin) return TDLO_OK;
    HIPCHK(c, drain_for_realloc(c));
    if (c->aln_dev) hipFree(c->aln_dev);
    if (c->aln_pin) hipHostFree(c->aln_pin);
    c->aln_dev = c->aln_pin = nullptr; c->aln_dev_cap = c->aln_pin_cap = 0; c->aln_armed = false;
    const size_t cap_c = std::max(Pc, c->aln_Pc), cap_d = std::max(Pd, c->aln_Pd);
    c->aln_Pc = c->aln_Pd = 0;
    const size_t dev_bytes = 256 + aln_round(4 * cap_c) + aln_round(2 * cap_c) + aln_round(2 * cap_d), pin_bytes = aln_round(2 * cap_d) + aln_round(2 * cap_c);
    HIPCHK(c, hipMalloc((void **)&c->aln_dev, dev_bytes));
    c->aln_dev_cap = dev_bytes;
    HIPCHK(c, hipHostMalloc((void **)&c->aln_pin, pin_bytes, hipHostMallocDefault));
    c->aln_pin_cap = pin_bytes; c->aln_Pc = cap_c; c->aln_Pd = cap_d;
    return TDLO_OK;
}

// What an align call refuses before it looks at the context's GPU: the params, the depth view
static int align_refusal(tdlo_ctx *c, const tdlo_image_view *depth, const tdlo_align_params *p) {
    if (const char *why = align_fault(p)) return fail(c, TDLO_E_INVALID, why);
    if (const char *why = image_view_fault(depth, p->rows_d, p->cols_d, kRoleDepth)) return fail(c, TDLO_E_INVALID, why);
    return TDLO_OK;
}

// The aligned plane of a checked (depth view, params), enqueued on the context's stream WITHOUT a host wait on the device route: *plane is the context's
// aligned plane.  The counts are the caller's after the stream's next wait (align_counts_fetch).  dev: where the depth view lies (image_view_where)
static int align_enqueue(tdlo_ctx *c, const tdlo_image_view *depth, bool dev, const tdlo_align_params *p, const unsigned short **plane) {
    HIPCHK(c, hipSetDevice(c->device));
    const size_t Pc = (size_t)p->rows_c * p->cols_c, Pd = (size_t)p->rows_d * p->cols_d;
    if (int rc = align_reserve(c, Pc, Pd)) return rc;
    if (dev && depth->ready_stream) {
        if (!c->ev_view) HIPCHK(c, hipEventCreateWithFlags(&c->ev_view, hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->ev_view, (hipStream_t)depth->ready_stream));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_view, 0));
    }
    *plane = aln_plane(c);
    if (c->align_host) {
        // the comparator: the host statement's plane, uploaded.  A device view comes down as its packed canonical depth (k_image_import, one copy, one wait)
        tdlo_image_view hv = *depth;
        if (dev) {
            ImageJob job{};
            job.P = (int)Pd; job.cols = p->cols_d;
            job.src[kRoleDepth] = ImageSrc{(const unsigned char *)depth->data, depth->row_stride, depth->format, image_import_form(depth->data, depth->row_stride, p->cols_d, depth->format)};
            job.dst[kRoleDepth] = (unsigned char *)aln_depth(c);
            HIPCHK(c, launch_image_import(job, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->aln_pin, aln_depth(c), 2 * Pd, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, wait_stream(c->stream));
            hv = tdlo_image_view{c->aln_pin, TDLO_IMG_U16C1, TDLO_MEM_HOST, 2ll * p->cols_d, nullptr};
        }
        long long n[4];
        if (tdlo_align_depth_host(&hv, p, aln_pin_plane(c), n)) return fail(c, TDLO_E_INVALID, "align: the host statement refused the call");
        for (int i = 0; i < 4; ++i) c->aln_res[4 + i] = (unsigned long long)n[i];
        HIPCHK(c, hipMemcpyAsync(aln_plane(c), aln_pin_plane(c), 2 * Pc, hipMemcpyHostToDevice, c->stream));
        c->aln_res_at = 4;
        ++c->aln_route[1];
        return TDLO_OK;
    }
    AlignJob job;
    align_job(depth, p, job);
    if (!dev) {                                             // a host view goes up once, packed
        image_pack_host(depth, p->rows_d, p->cols_d, c->aln_pin);
        HIPCHK(c, hipMemcpyAsync(aln_depth(c), c->aln_pin, 2 * Pd, hipMemcpyHostToDevice, c->stream));
        job.depth = (const unsigned char *)aln_depth(c); job.row_stride = 2ll * p->cols_d; job.format = TDLO_IMG_U16C1;
    }
    if (!c->aln_armed) {                                    // the first use of an allocation (or after a call that failed between its launches): filled once
        HIPCHK(c, hipMemsetAsync(c->aln_dev, 0, 256, c->stream));
        HIPCHK(c, hipMemsetAsync(aln_scratch(c), 0xff, 4 * c->aln_Pc, c->stream));
    }
    c->aln_armed = false;
    HIPCHK(c, launch_align(job, aln_scratch(c), aln_plane(c), aln_counts(c), c->aln_res, c->stream));
    c->aln_armed = true;                                    // k_align_pack leaves every word it read, and the counts, armed
    c->aln_res_at = 0;
    ++c->aln_route[0];
    return TDLO_OK;
}

// after a wait of the context's stream that followed align_enqueue
static void align_counts_fetch(tdlo_ctx *c, long long counts[4]) {
    if (counts) for (int i = 0; i < 4; ++i) counts[i] = (long long)c->aln_res[c->aln_res_at + i];
}

int tdlo_align_depth(tdlo_ctx *c, const tdlo_image_view *depth, const tdlo_align_params *p, unsigned short *aligned_out,
                     const unsigned short **device_plane, long long counts[4]) {
    if (!c) return TDLO_E_INVALID;
    int rc = align_refusal(c, depth, p);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    bool dev = false, out_dev = false;
    if ((rc = image_view_where(c, depth, p->rows_d, p->cols_d, &dev))) return rc;
    if (aligned_out && (rc = pointer_location(c, aligned_out, TDLO_MEM_AUTO, "align: aligned_out", &out_dev))) return rc;
    const unsigned short *plane = nullptr;
    if ((rc = align_enqueue(c, depth, dev, p, &plane))) { (void)hipStreamSynchronize(c->stream); return rc; }
    const size_t bytes = 2 * (size_t)p->rows_c * p->cols_c;
    if (aligned_out) HIPCHK(c, hipMemcpyAsync(aligned_out, plane, bytes, out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, wait_stream(c->stream));
    align_counts_fetch(c, counts);
    if (device_plane) *device_plane = plane;
    return TDLO_OK;
}

// The checks of an aligning frame call, in front of everything it touches: the params and the depth view at the depth camera's size, the rest of the frame
// at the colour camera's (fv2: the frame the view call behind it will see, its depth a device view of the aligned plane), where every view lies
static int align_frame_refusal(tdlo_ctx *c, int slot, const tdlo_frame_view *fv, const tdlo_align_params *p, const tdlo_colour_params *cp, double leaf_size,
                               tdlo_frame_view &fv2, bool *depth_dev) {
    if (!fv) return fail(c, TDLO_E_INVALID, "frame view: null");
    int rc = align_refusal(c, &fv->depth, p);
    if (rc) return rc;
    alignas(8) static const unsigned short placeholder[4] = {0, 0, 0, 0};      // stands for the aligned plane until it exists
    fv2 = *fv;
    fv2.depth = tdlo_image_view{placeholder, TDLO_IMG_U16C1, TDLO_MEM_DEVICE, 2ll * p->cols_c, nullptr};
    if ((rc = frame_view_refusal(c, slot, &fv2, cp, p->rows_c, p->cols_c, p->fx_c, p->fy_c, leaf_size))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = image_view_where(c, &fv->depth, p->rows_d, p->cols_d, depth_dev))) return rc;
    const tdlo_image_view *iv[3] = {&fv->colour, &fv->occluder, &fv->mask};
    for (int r = 0; r < 3; ++r) {
        bool d;
        if (iv[r]->data && (rc = image_view_where(c, iv[r], p->rows_c, p->cols_c, &d))) return rc;
    }
    return TDLO_OK;
}

int tdlo_frame_to_cloud_view_aligning(tdlo_ctx *c, int slot, const tdlo_frame_view *fv, const tdlo_align_params *p, const tdlo_colour_params *colour_params,
                                      double leaf_size, double *X_out, int x_capacity, int *n_out, int *n_raw_out, long long counts[4]) {
    if (!c) return TDLO_E_INVALID;
    tdlo_frame_view fv2;
    bool dev = false;
    int rc = align_frame_refusal(c, slot, fv, p, colour_params, leaf_size, fv2, &dev);
    if (rc) return rc;
    const unsigned short *plane = nullptr;
    StagedFrame sf;
    if ((rc = align_enqueue(c, &fv->depth, dev, p, &plane)) || (fv2.depth.data = plane, rc = stage_frame_view(c, &fv2, colour_params, p->rows_c, p->cols_c, sf))) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    rc = depth_to_cloud_impl(c, slot, sf.depth, sf.mask, p->rows_c, p->cols_c, p->fx_c, p->fy_c, p->cx_c, p->cy_c, leaf_size, X_out, x_capacity, n_out, n_raw_out,
                             nullptr, 0, nullptr, sf.colour ? &sf.ci : nullptr);
    if (rc) (void)hipStreamSynchronize(c->stream);
    align_counts_fetch(c, counts);
    return rc;
}

// ---- image views for F slots in one call (include/trackdlo_hip.h: tdlo_frame_views_to_cloud_batch) ------------------------------------------------
// From this many frames on the calls are the batch launches; below it they loop over the single view calls (the same bits).  The rule, set beforehand, is the
// packed batch's: the smallest F from which every batch value lies below every single-calls value on the lines a call stands for, at both image sizes
// (scripts/gpu_frame_view_batch.py -> profiles/frame_view_batch_ab.txt); the cloud call and the tracker call take separate constants.  33 = off by default.
// Measured against the parent commit's library: device views win on every value from 2 frames at 640 x 480 and from 4 at 1280 x 720 (32 RGBA8 + 32FC1
// images 0.20 against 1.42 ms and 0.58 against 1.83 ms), but F host views, packed into the pinned block and copied up, stay behind F single calls that read
// the context's pinned image buffers in place at 1280 x 720 at every F (9.6 against 7.3 ms at 32) -- what happened to the packed batch -- so the cloud call
// is OFF by default.  The tracker call (device views) wins on every value from 4 trackers on at both sizes (32 trackers 2.13 against 5.69 ms and 2.29
// against 5.74 ms).  TDLO_FRAME_VIEW_BATCH_MIN=n, read when the context is made, overrides both.
constexpr int kFrameViewBatchMin = 33;
constexpr int kFrameViewBatchTrackerMin = 4;
static int frame_view_batch_min(const tdlo_ctx *c, bool tracker) {
    return c->frame_view_batch_min ? c->frame_view_batch_min : (tracker ? kFrameViewBatchTrackerMin : kFrameViewBatchMin);
}

// [a0, a1) of a checked view
static void image_view_bytes(const tdlo_image_view *v, int rows, int cols, const char **a0, const char **a1) {
    long long lo, hi;
    image_view_span(v, rows, cols, &lo, &hi);
    *a0 = (const char *)v->data + lo; *a1 = (const char *)v->data + hi;
}

struct ViewImageWhere { bool dev[4] = {false, false, false, false}; };      // by role: depth, colour, occluder, mask

// Everything that refuses the call as a whole; nothing of the context or the slots is touched.  where: per image, which of its views lie in device memory.
static int frame_views_batch_refusal(tdlo_ctx *c, const tdlo_view_image *images, int K, int rows, int cols, const tdlo_batch_frame *frames, int F, double leaf_size,
                                     std::vector<ViewImageWhere> &where) {
    where.assign(images && K >= 1 ? K : 0, ViewImageWhere{});
    int rc = cloud_batch_refusal_common(c, images != nullptr, K, rows, cols, frames, F, leaf_size, [&](int k, BatchImageHas &h) -> int {
        const tdlo_view_image &im = images[k];
        const tdlo_image_view *iv[4] = {&im.fv.depth, &im.fv.colour, &im.fv.occluder, &im.fv.mask};
        h = BatchImageHas{im.fv.depth.data != nullptr, im.fv.mask.data != nullptr, im.fv.colour.data != nullptr, im.fx, im.fy};
        if (!h.depth || (!h.mask && !h.colour)) return fail(c, TDLO_E_INVALID, "cloud batch: an image needs depth and a mask or a colour image");
        if (im.fv.occluder.data && !h.colour) return fail(c, TDLO_E_INVALID, "frame view: an occluder goes with a colour image, not with a mask");
        if (im.fx == 0 || im.fy == 0) return fail(c, TDLO_E_INVALID, "bad leaf size / intrinsics");
        for (int r = 0; r < 4; ++r) {
            if (!iv[r]->data) continue;
            if (const char *why = image_view_fault(iv[r], rows, cols, r)) return fail(c, TDLO_E_INVALID, why);
            if (int e = pointer_location(c, iv[r]->data, iv[r]->location, "image view", &where[k].dev[r])) return e;
            const char *a0, *a1;
            image_view_bytes(iv[r], rows, cols, &a0, &a1);
            auto hits = [&](const void *p, size_t bytes) { return p && a0 < (const char *)p + bytes && (const char *)p < a1; };
            if (!where[k].dev[r]) {
                if (hits(c->img_pin, c->img_pin_cap) || hits(c->col_pin, c->col_pin_cap))
                    return fail(c, TDLO_E_INVALID, "image view: a host view inside the context's pinned image buffers (hand those to the packed calls)");
            } else if (hits(c->cbat_dev, c->cbat_dev_cap) || hits(c->cbat_img, c->cbat_img_cap))
                return fail(c, TDLO_E_INVALID, "frame view batch: a device view overlaps the batch arena");
        }
        return TDLO_OK;
    });
    if (rc) return rc;
    for (int k = 0; k < K; ++k) {
        const tdlo_image_view *iv[4] = {&images[k].fv.depth, &images[k].fv.colour, &images[k].fv.occluder, &images[k].fv.mask};
        for (int r = 0; r < 4; ++r) {
            if (!iv[r]->data || !where[k].dev[r]) continue;
            const char *a0, *a1;
            image_view_bytes(iv[r], rows, cols, &a0, &a1);
            for (int f = 0; f < F; ++f) {
                const Slot &s = c->slots[frames[f].slot];
                const char *x0 = (const char *)s.Xraw, *x1 = x0 + 3 * (size_t)s.cap_points * sizeof(double);
                if (s.Xraw && a0 < x1 && x0 < a1) return fail(c, TDLO_E_INVALID, "frame view batch: a device view overlaps the resident cloud of a slot the call names");
            }
        }
    }
    return TDLO_OK;
}

// tracker: the call stands behind the tracker entrance (frame_view_batch_min)
static int frame_views_batch_impl(tdlo_ctx *c, const tdlo_view_image *images, int K, int rows, int cols, const tdlo_batch_frame *frames, int F, double leaf_size,
                                  int *n_out, int *n_raw_out, int *rc_each, bool tracker) {
    if (!c) return TDLO_E_INVALID;
    std::vector<ViewImageWhere> where;
    int rc = frame_views_batch_refusal(c, images, K, rows, cols, frames, F, leaf_size, where);
    if (rc) return rc;
    std::vector<int> n(F, 0), nraw(F, 0), rcs(F, 0);
    auto finish = [&]() {
        if (n_out) std::copy(n.begin(), n.end(), n_out);
        if (n_raw_out) std::copy(nraw.begin(), nraw.end(), n_raw_out);
        if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
        for (int f = 0; f < F; ++f) if (rcs[f]) return rcs[f];
        return (int)TDLO_OK;
    };
    // one frame through the single view call: the views it reads, and no others
    auto single = [&](int f) {
        const tdlo_view_image &im = images[frames[f].image];
        tdlo_frame_view one{};
        one.depth = im.fv.depth;
        if (frames[f].colour_params) { one.colour = im.fv.colour; one.occluder = im.fv.occluder; }
        else one.mask = im.fv.mask;
        return tdlo_frame_to_cloud_view(c, frames[f].slot, &one, frames[f].colour_params, rows, cols, im.fx, im.fy, im.cx, im.cy, leaf_size, nullptr, 0, &n[f], &nraw[f]);
    };
    const int P = rows * cols;
    if (F < frame_view_batch_min(c, tracker) || !c->cloud_fused_on || !cloud_fused_ok(P)) {
        c->fvbat_planes.assign(K, tdlo_ctx::ViewBatchPlanes{{nullptr, nullptr, nullptr, nullptr}});      // (a view batch that imported nothing into the arena)
        for (int f = 0; f < F; ++f) { ++c->fvbat_route[1]; rcs[f] = single(f); }
        return finish();
    }
    // ---- the views the frames read, every distinct (data, format, row_stride, role) once: the host views first (their part of the plane region goes up in
    // one copy from a pinned block laid out the same), then the device views (written by the import launch)
    const size_t plane_bytes[4] = {img_depth_bytes(P), img_colour_bytes(P), img_occ_bytes(P), img_mask_bytes(P)};
    std::vector<char> use(4 * (size_t)K, 0);
    for (int f = 0; f < F; ++f) {
        const int k = frames[f].image;
        use[4 * k + kRoleDepth] = 1;
        if (frames[f].colour_params) { use[4 * k + kRoleColour] = 1; if (images[k].fv.occluder.data) use[4 * k + kRoleOccluder] = 1; }
        else use[4 * k + kRoleMask] = 1;
    }
    struct Plane { const tdlo_image_view *v; int role; bool dev; size_t off; int image; };
    std::vector<Plane> planes;
    std::vector<size_t> at(4 * (size_t)K, kNoPlane);
    size_t img_bytes = 0, host_bytes = 0;
    int dev_planes = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int k = 0; k < K; ++k) {
            const tdlo_image_view *iv[4] = {&images[k].fv.depth, &images[k].fv.colour, &images[k].fv.occluder, &images[k].fv.mask};
            for (int r = 0; r < 4; ++r) {
                if (!use[4 * k + r] || where[k].dev[r] != (pass == 1)) continue;
                size_t j = 0;
                while (j < planes.size() && !(planes[j].role == r && planes[j].v->data == iv[r]->data && planes[j].v->format == iv[r]->format && planes[j].v->row_stride == iv[r]->row_stride)) ++j;
                if (j == planes.size()) { planes.push_back(Plane{iv[r], r, pass == 1, img_bytes, k}); img_bytes += plane_bytes[r]; dev_planes += pass; }
                at[4 * k + r] = planes[j].off;
            }
        }
        if (pass == 0) host_bytes = img_bytes;
    }
    // a job of the import launch is one image: the device views it is the first to name
    std::vector<int> job_of(K, -1);
    int J = 0;
    for (const Plane &pl : planes) if (pl.dev && job_of[pl.image] < 0) job_of[pl.image] = J++;
    auto r256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t tab2 = r256(sizeof(ImageJob) * (size_t)J);
    std::vector<CloudBatchIn> in(F);
    for (int f = 0; f < F; ++f) {
        const int k = frames[f].image;
        const tdlo_view_image &im = images[k];
        in[f] = CloudBatchIn{frames[f].slot, at[4 * k + kRoleDepth], at[4 * k + kRoleMask], at[4 * k + kRoleColour],
                             frames[f].colour_params ? at[4 * k + kRoleOccluder] : kNoPlane, frames[f].colour_params, {im.fx, im.fy, im.cx, im.cy}};
    }
    hipStream_t st = c->stream;
    char *d_img = nullptr;
    const CloudBatchEnqueue enqueue = [&](const CloudBatchArena &ar, const CloudBatchFrame *bf, int Fm, int Fc, float inv, unsigned epoch) -> int {
        d_img = ar.d_img;
        ImageJob *jobs = (ImageJob *)ar.h_tab2;
        for (int j = 0; j < J; ++j) { jobs[j] = ImageJob{}; jobs[j].P = P; jobs[j].cols = cols; }
        for (const Plane &pl : planes) {
            if (!pl.dev) { image_pack_host(pl.v, rows, cols, ar.h_tail + pl.off); continue; }
            ImageJob &job = jobs[job_of[pl.image]];
            job.src[pl.role] = ImageSrc{(const unsigned char *)pl.v->data, pl.v->row_stride, pl.v->format, image_import_form(pl.v->data, pl.v->row_stride, cols, pl.v->format)};
            job.dst[pl.role] = (unsigned char *)ar.d_img + pl.off;
        }
        HIPCHK(c, cloud_fused_batch_table(bf, Fm, Fc, P, cols, inv, epoch, ar.h_tab));
        // the context's stream waits for what the device views' ready_streams hold so far: one event per distinct stream
        std::vector<void *> seen;
        for (int k = 0; k < K; ++k) {
            const tdlo_image_view *iv[4] = {&images[k].fv.depth, &images[k].fv.colour, &images[k].fv.occluder, &images[k].fv.mask};
            for (int r = 0; r < 4; ++r) {
                void *rs = iv[r]->ready_stream;
                if (!use[4 * k + r] || !where[k].dev[r] || !rs || std::find(seen.begin(), seen.end(), rs) != seen.end()) continue;
                if (seen.size() >= c->wbat_ev.size()) {
                    hipEvent_t e = nullptr;
                    HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
                    c->wbat_ev.push_back(e);
                }
                hipEvent_t e = c->wbat_ev[seen.size()];
                HIPCHK(c, hipEventRecord(e, (hipStream_t)rs));
                HIPCHK(c, hipStreamWaitEvent(st, e, 0));
                seen.push_back(rs);
            }
        }
        // ONE copy: the descriptor table, the job table and the host views' planes, which lie behind one another on both sides
        HIPCHK(c, hipMemcpyAsync(ar.d_tab, ar.h_tab, (size_t)(ar.h_tail - ar.h_tab) + host_bytes, hipMemcpyHostToDevice, st));
        if (J > 0) {
            HIPCHK(c, launch_image_import_batch(jobs, J, ar.d_tab2, st));
            c->fvbat_route[2] += dev_planes;
        }
        HIPCHK(c, launch_cloud_fused_batch_tabled(Fm, Fc, P, ar.d_tab, st));
        return TDLO_OK;
    };
    std::vector<int> passed;
    if ((rc = cloud_batch_run(c, in, P, leaf_size, tab2, img_bytes, host_bytes, enqueue, c->fvbat_route, n, nraw, rcs, passed))) return rc;
    c->fvbat_planes.assign(K, tdlo_ctx::ViewBatchPlanes{{nullptr, nullptr, nullptr, nullptr}});
    for (int k = 0; k < K; ++k)
        for (int r = 0; r < 4; ++r)
            if (at[4 * k + r] != kNoPlane) c->fvbat_planes[k].p[r] = d_img + at[4 * k + r];
    for (int f : passed) rcs[f] = single(f);                  // (cloud_batch_run has counted them)
    return finish();
}

int tdlo_frame_views_to_cloud_batch(tdlo_ctx *c, const tdlo_view_image *images, int K, int rows, int cols, const tdlo_batch_frame *frames, int F, double leaf_size,
                                    int *n_out, int *n_raw_out, int *rc_each) {
    return frame_views_batch_impl(c, images, K, rows, cols, frames, F, leaf_size, n_out, n_raw_out, rc_each, false);
}

int tdlo_view_batch_images(tdlo_ctx *c, int k, const unsigned short **depth, const unsigned char **colour, const unsigned char **occluder, const unsigned char **mask) {
    if (!c) return TDLO_E_INVALID;
    if (c->fvbat_planes.empty()) return fail(c, TDLO_E_INVALID, "tdlo_view_batch_images: no view batch since the arena was last written");
    if (k < 0 || k >= (int)c->fvbat_planes.size()) return fail(c, TDLO_E_INVALID, "tdlo_view_batch_images: image index out of range");
    const tdlo_ctx::ViewBatchPlanes &pl = c->fvbat_planes[k];
    if (depth) *depth = (const unsigned short *)pl.p[kRoleDepth];
    if (colour) *colour = (const unsigned char *)pl.p[kRoleColour];
    if (occluder) *occluder = (const unsigned char *)pl.p[kRoleOccluder];
    if (mask) *mask = (const unsigned char *)pl.p[kRoleMask];
    return TDLO_OK;
}

int tdlo_debug_slot_cloud(tdlo_ctx *c, int slot, const double **X, int *capacity) {
    if (!c) return TDLO_E_INVALID;
    if (slot < 0 || slot >= (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "bad slot");
    if (X) *X = c->slots[slot].Xraw;
    if (capacity) *capacity = c->slots[slot].Xraw ? c->slots[slot].cap_points : 0;
    return TDLO_OK;
}

int tdlo_debug_read_images(tdlo_ctx *c, int rows, int cols, unsigned short *depth_out, unsigned char *colour_out, unsigned char *occluder_out,
                           unsigned char *mask_out) {
    if (!c) return TDLO_E_INVALID;
    if (c->view_rows != rows || c->view_cols != cols || rows <= 0 || cols <= 0) return fail(c, TDLO_E_INVALID, "tdlo_debug_read_images: no view call of this shape yet");
    void *out[4] = {depth_out, colour_out, occluder_out, mask_out};
    const size_t P = (size_t)rows * cols, bytes[4] = {2 * P, 3 * P, P, P};
    for (int r = 0; r < 4; ++r)
        if (out[r] && !c->view_img[r]) return fail(c, TDLO_E_INVALID, "tdlo_debug_read_images: the last view frame had no such image");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int r = 0; r < 4; ++r)
        if (out[r]) HIPCHK(c, hipMemcpy(out[r], c->view_img[r], bytes[r], hipMemcpyDefault));
    return TDLO_OK;
}

// ---- measurement ---------------------------------------------------------------------------------
int tdlo_profile_kernel(tdlo_ctx *c, int slot, int kind, int reps, float *avg_us) {
    if (!c || c->last_F < 1 || c->fh.empty()) return TDLO_E_INVALID;
    if (!((kind >= 0 && kind <= 4) || kind == 10) || reps < 1 || (kind == 10 && reps > 256)) return fail(c, TDLO_E_INVALID, "bad kind / reps");
    (void)slot;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int F = c->last_F;
    // the loop left done = 1; clear it so the kernels do their work (state is scratch from here on)
    std::vector<IterState> saved(F);
    for (int i = 0; i < F; ++i) {
        HIPCHK(c, hipMemcpyAsync(&saved[i], c->fh[i].st, sizeof(IterState), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipStreamSynchronize(s));
    for (int i = 0; i < F; ++i) {
        IterState is = saved[i];
        is.done = 0; is.it = 0;
        std::memcpy(c->pin + i * 16, &is, sizeof is);
        HIPCHK(c, hipMemcpyAsync(c->fh[i].st, c->pin + i * 16, sizeof(IterState), hipMemcpyHostToDevice, s));
    }
    std::vector<FrameDev> fh = c->fh;
    for (auto &f : fh) f.max_iter = 1 << 30;
    for (auto &f : fh) f.tol = -1.0;
    HIPCHK(c, hipMemcpyAsync(c->fd, fh.data(), sizeof(FrameDev) * F, hipMemcpyHostToDevice, s));
    HIPCHK(c, zero_accumulators(fh, F, s));
    if (kind == 10) {
        // E-step in situ: real iterations (E-step, M-step alternating, as in the loop), every E-step dispatch carries its
        // own start/stop events -- the duration a kernel trace reports, not a back-to-back average with hot caches
        std::vector<hipEvent_t> evs(2 * (size_t)reps, nullptr);
        for (auto &e : evs) HIPCHK(c, hipEventCreate(&e));
        for (int w = 0; w < 3; ++w) HIPCHK(c, launch_iteration(c->fd, fh.data(), F, s, w));      // (the counter was set to 0 above)
        for (int r = 0; r < reps; ++r) HIPCHK(c, launch_iteration_timed(c->fd, fh.data(), F, s, evs[2 * r], evs[2 * r + 1], nullptr, nullptr, 3 + r));
        HIPCHK(c, hipStreamSynchronize(s));
        double tot = 0;
        for (int r = 0; r < reps; ++r) { float ms = 0; hipEventElapsedTime(&ms, evs[2 * r], evs[2 * r + 1]); tot += ms; }
        for (auto &e : evs) hipEventDestroy(e);
        if (avg_us) *avg_us = (float)(tot * 1000.0 / reps);
    } else {
    if (kind >= 2) {
        // M-step kinds: every repetition needs this iteration's sums, which an M-step consumes (it clears the other parity's rows and
        // advances the iteration counter) -- so the E-step runs in between, outside the timed spans (one event pair per repetition)
        std::vector<hipEvent_t> evs(2 * (size_t)reps, nullptr);
        for (auto &e : evs) HIPCHK(c, hipEventCreate(&e));
        double tot = 0;
        for (int r = -3; r < reps; ++r) {
            if (fh[0].vis_branch) HIPCHK(c, launch_estep_only(c->fd, fh.data(), F, 1, s));
            HIPCHK(c, launch_estep_only(c->fd, fh.data(), F, 0, s));
            if (kind == 4) HIPCHK(c, launch_estep_only(c->fd, fh.data(), F, 3, s));      // the sums this kind starts from
            if (r >= 0) HIPCHK(c, hipEventRecord(evs[2 * r], s));
            HIPCHK(c, launch_estep_only(c->fd, fh.data(), F, kind, s));
            if (r >= 0) HIPCHK(c, hipEventRecord(evs[2 * r + 1], s));
            if (kind == 3) HIPCHK(c, launch_estep_only(c->fd, fh.data(), F, 4, s));      // export only: finish the iteration
        }
        HIPCHK(c, hipStreamSynchronize(s));
        for (int r = 0; r < reps; ++r) { float ms = 0; hipEventElapsedTime(&ms, evs[2 * r], evs[2 * r + 1]); tot += ms; }
        for (auto &e : evs) hipEventDestroy(e);
        if (avg_us) *avg_us = (float)(tot * 1000.0 / reps);
    } else {
    for (int w = 0; w < 3; ++w) HIPCHK(c, launch_estep_only(c->fd, fh.data(), F, kind, s));
    HIPCHK(c, hipEventRecord(c->ev[0], s));
    for (int r = 0; r < reps; ++r) HIPCHK(c, launch_estep_only(c->fd, fh.data(), F, kind, s));
    HIPCHK(c, hipEventRecord(c->ev[1], s));
    HIPCHK(c, hipStreamSynchronize(s));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
    if (avg_us) *avg_us = ms * 1000.0f / (float)reps;
    }
    }
    HIPCHK(c, zero_accumulators(fh, F, s));
    // restore
    for (int i = 0; i < F; ++i) {
        std::memcpy(c->pin + i * 16, &saved[i], sizeof(IterState));
        HIPCHK(c, hipMemcpyAsync(c->fh[i].st, c->pin + i * 16, sizeof(IterState), hipMemcpyHostToDevice, s));
    }
    HIPCHK(c, hipMemcpyAsync(c->fd, c->fh.data(), sizeof(FrameDev) * F, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return TDLO_OK;
}

int tdlo_profile_iteration(tdlo_ctx *c, int reps, float *estep_us, float *mstep_us, float *iter_us, char *mstep_kernel, int name_cap) {
    if (!c || c->last_F < 1 || c->fh.empty()) return TDLO_E_INVALID;
    if (reps < 1 || reps > 256) return fail(c, TDLO_E_INVALID, "bad reps");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int F = c->last_F;
    std::vector<IterState> saved(F);
    for (int i = 0; i < F; ++i) HIPCHK(c, hipMemcpyAsync(&saved[i], c->fh[i].st, sizeof(IterState), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (int i = 0; i < F; ++i) {
        IterState is = saved[i];
        is.done = 0; is.it = 0;
        std::memcpy(c->pin + i * 16, &is, sizeof is);
        HIPCHK(c, hipMemcpyAsync(c->fh[i].st, c->pin + i * 16, sizeof(IterState), hipMemcpyHostToDevice, s));
    }
    std::vector<FrameDev> fh = c->fh;
    for (auto &f : fh) { f.max_iter = 1 << 30; f.tol = -1.0; }
    HIPCHK(c, hipMemcpyAsync(c->fd, fh.data(), sizeof(FrameDev) * F, hipMemcpyHostToDevice, s));
    HIPCHK(c, zero_accumulators(fh, F, s));
    std::vector<hipEvent_t> evs(4 * (size_t)reps, nullptr);
    for (auto &e : evs) HIPCHK(c, hipEventCreate(&e));
    for (int w = 0; w < 3; ++w) HIPCHK(c, launch_iteration(c->fd, fh.data(), F, s, w));      // (the counter was set to 0 above)
    HIPCHK(c, hipEventRecord(c->ev[0], s));
    for (int r = 0; r < reps; ++r) HIPCHK(c, launch_iteration_timed(c->fd, fh.data(), F, s, evs[4 * r], evs[4 * r + 1], evs[4 * r + 2], evs[4 * r + 3], 3 + r));
    HIPCHK(c, hipEventRecord(c->ev[1], s));
    HIPCHK(c, hipStreamSynchronize(s));
    double te = 0, tm = 0;
    bool m_ok = true;
    for (int r = 0; r < reps; ++r) {
        float ms = 0;
        hipEventElapsedTime(&ms, evs[4 * r], evs[4 * r + 1]); te += ms;
        if (hipEventElapsedTime(&ms, evs[4 * r + 2], evs[4 * r + 3]) == hipSuccess) tm += ms; else m_ok = false;     // dispatch without events
    }
    (void)hipGetLastError();
    float tot = 0;
    hipEventElapsedTime(&tot, c->ev[0], c->ev[1]);
    for (auto &e : evs) hipEventDestroy(e);
    if (estep_us) *estep_us = (float)(te * 1000.0 / reps);
    if (mstep_us) *mstep_us = m_ok ? (float)(tm * 1000.0 / reps) : -1.0f;
    if (iter_us) *iter_us = tot * 1000.0f / (float)reps;
    if (mstep_kernel && name_cap > 0) { std::strncpy(mstep_kernel, mstep_kernel_name(fh.data(), F), (size_t)name_cap - 1); mstep_kernel[name_cap - 1] = 0; }
    for (int i = 0; i < F; ++i) {
        std::memcpy(c->pin + i * 16, &saved[i], sizeof(IterState));
        HIPCHK(c, hipMemcpyAsync(c->fh[i].st, c->pin + i * 16, sizeof(IterState), hipMemcpyHostToDevice, s));
    }
    HIPCHK(c, zero_accumulators(fh, F, s));
    HIPCHK(c, hipMemcpyAsync(c->fd, c->fh.data(), sizeof(FrameDev) * F, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return TDLO_OK;
}

int tdlo_debug_read_cloud(tdlo_ctx *c, int frame, double *out, int max_points, double *ctr) {
    if (!c || frame < 0 || frame >= (int)c->fh.size() || !out) return TDLO_E_INVALID;
    const FrameDev &f = c->fh[frame];
    IterState is;
    HIPCHK(c, hipMemcpy(&is, f.st, sizeof is, hipMemcpyDeviceToHost));
    const int N = is.N;
    if (N > max_points) return TDLO_E_INVALID;
    const size_t es = f.precision == TDLO_PREC_F64 ? 8 : 4;
    std::vector<char> buf(es * (size_t)N);
    for (int d = 0; d < 3; ++d) {
        HIPCHK(c, hipMemcpy(buf.data(), (const char *)f.Xs + es * (size_t)f.ldx * d, es * (size_t)N, hipMemcpyDeviceToHost));
        for (int n = 0; n < N; ++n) out[(size_t)d * N + n] = es == 8 ? ((const double *)buf.data())[n] : (double)((const float *)buf.data())[n];
    }
    if (ctr) HIPCHK(c, hipMemcpy(ctr, f.ctr, 3 * sizeof(double), hipMemcpyDeviceToHost));
    return N;
}

int tdlo_debug_read_setup(tdlo_ctx *c, int frame, int what, double *out, int cap) {
    if (!c || frame < 0 || frame >= (int)c->fh.size() || !out) return TDLO_E_INVALID;
    const FrameDev &f = c->fh[frame];
    const int M = f.M;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double *src = nullptr;
    int n = 0;
    switch (what) {
    case TDLO_SETUP_COORD: src = f.coord; n = M; break;
    case TDLO_SETUP_CHAIN: src = f.chain; n = 8 * M; break;
    case TDLO_SETUP_HY0: src = f.include_lle ? f.HY0 : nullptr; n = 3 * M; break;
    case TDLO_SETUP_Y0: src = f.Y0; n = 3 * M; break;
    case TDLO_SETUP_NODES: {
        n = 4 * M;
        if (n > cap || !f.nodes) return TDLO_E_INVALID;
        if (f.precision == TDLO_PREC_F64) { HIPCHK(c, hipMemcpy(out, f.nodes, sizeof(double) * n, hipMemcpyDeviceToHost)); return n; }
        std::vector<float> buf((size_t)n);
        HIPCHK(c, hipMemcpy(buf.data(), f.nodes, sizeof(float) * n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) out[i] = (double)buf[i];
        return n;
    }
    case TDLO_SETUP_KEEP: {
        n = 4;
        if (n > cap || !f.keep || !f.st) return TDLO_E_INVALID;
        IterState is;
        HIPCHK(c, hipMemcpy(out, f.keep, 2 * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&is, f.st, sizeof is, hipMemcpyDeviceToHost));
        out[2] = (double)is.N; out[3] = is.sum_d2;
        return n;
    }
    case TDLO_SETUP_SIGMA2: {
        n = 1;
        if (n > cap || !f.st) return TDLO_E_INVALID;
        IterState is;
        HIPCHK(c, hipMemcpy(&is, f.st, sizeof is, hipMemcpyDeviceToHost));
        out[0] = is.sigma2;
        return n;
    }
    default: return TDLO_E_INVALID;
    }
    if (!src || n > cap) return TDLO_E_INVALID;
    HIPCHK(c, hipMemcpy(out, src, sizeof(double) * n, hipMemcpyDeviceToHost));
    return n;
}

int tdlo_debug_mstep_dense(int on) { return mstep_set_dense(on); }
int tdlo_debug_mstep_lle_dense(int on) { return mstep_set_lle_dense(on); }
long long tdlo_debug_band_retries(tdlo_ctx *c) { return c ? c->band_retries : -1; }

long long tdlo_debug_route_count(tdlo_ctx *c, int which) {
    if (!c || which < 0 || which > 63) return -1;
    if (which >= 59) return c->aln_route[which - 59];
    if (which >= 57) return c->cel_route[which - 57];
    if (which >= 55) return c->clu_route[which - 55];
    if (which >= 53) return c->asg_route[which - 53];
    if (which >= 51) return c->pnt_route[which - 51];
    if (which >= 49) return c->rbatch_route[which - 49];
    if (which == 48) return c->prologue_scan_calls;
    if (which >= 45) return c->rig_route[which - 45];
    if (which >= 42) return c->fvbat_route[which - 42];
    if (which >= 38) return c->wbat_route[which - 38];
    if (which >= 36) return c->ibat_route[which - 36];
    if (which >= 34) return c->rbat_route[which - 34];
    if (which >= 32) return c->cbat_route[which - 32];
    if (which >= 30) return c->vbat_route[which - 30];
    if (which >= 27) return c->view_team_route[which - 27];
    if (which >= 25) return c->init_route[which - 25];
    if (which == 24) return c->fused_w0_calls;
    if (which >= 22) return c->vis_route[which - 22];
    if (which == 21) return c->voxel_view_calls;
    if (which >= 19) return c->render_route[which - 19];
    if (which >= 17) return c->view_route[which - 17];
    if (which >= 15) return c->colour_route[which - 15];
    if (which == 14) return c->fused_calls;
    if (which >= 11 && which <= 13) return 0;      // (belonged to experiments that were removed; not reused)
    if (which == 10) return c->boost_retries;
    if (which == 9) return c->estep2_frames;
    if (which == 8) return c->cloud_vis_rides;
    return which < 6 ? c->route_count[which] : c->cloud_route[which - 6];
}

int tdlo_debug_lle_band_device(tdlo_ctx *c, const double *Y, int M, double *Hb) {
    if (!c) return TDLO_E_INVALID;
    if (!Y || !Hb || M < 1 || M > 256) return fail(c, TDLO_E_INVALID, "tdlo_debug_lle_band_device: 1 .. 256 nodes");
    HIPCHK(c, hipSetDevice(c->device));
    double *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, sizeof(double) * 16 * (size_t)M));
    hipError_t e = hipMemcpyAsync(d, Y, sizeof(double) * 3 * M, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_lle_band_debug(d, M, d + 3 * M, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(Hb, d + 3 * M, sizeof(double) * 13 * M, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    HIPCHK(c, e);
    return TDLO_OK;
}
int tdlo_debug_fail_hip(tdlo_ctx *c) {
    if (!c) return TDLO_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(nullptr, nullptr, 16, hipMemcpyDeviceToDevice));      // hipErrorInvalidValue
    return TDLO_OK;
}

int tdlo_pci_bus_id(tdlo_ctx *c, char *out, int len) {
    if (!c || !out || len < 16) return TDLO_E_INVALID;
    HIPCHK(c, hipDeviceGetPCIBusId(out, len, c->device));
    return TDLO_OK;
}

int tdlo_set_xch_self(tdlo_ctx *c, int on) {
    if (!c) return TDLO_E_INVALID;
    const int prev = c->xch_self ? 1 : 0;
    c->xch_self = on != 0;
    return prev;
}

int tdlo_set_sort_reuse(tdlo_ctx *c, int on) {
    if (!c) return TDLO_E_INVALID;
    const int prev = c->sort_reuse ? 1 : 0;
    c->sort_reuse = on != 0;
    return prev;
}

int tdlo_set_timing(tdlo_ctx *c, int on) {
    if (!c) return TDLO_E_INVALID;
    const int prev = c->timing ? 1 : 0;
    c->timing = on != 0;
    return prev;
}

int tdlo_debug_stamps(tdlo_ctx *c, int slot, unsigned long long *out, int n) {
    if (!c || slot < 0 || slot >= (int)c->slots.size() || !out || n < 1 || n > 64 || c->fh.empty()) return TDLO_E_INVALID;
    const int dbg_frame = getenv("TDLO_DEBUG_FRAME") ? atoi(getenv("TDLO_DEBUG_FRAME")) : 0;      // which frame of the last batch
    if (dbg_frame < 0 || dbg_frame >= (int)c->fh.size()) return TDLO_E_INVALID;
    HIPCHK(c, hipMemcpyAsync(c->pin, c->fh[dbg_frame].dbg, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(out, c->pin, sizeof(unsigned long long) * n);
    return TDLO_OK;
}

int tdlo_debug_cloud_stamps(tdlo_ctx *c, unsigned long long *out, int n) {
    if (!c || !out || n < 0 || n > 24) return TDLO_E_INVALID;
    if (!c->cloud_fws) return fail(c, TDLO_E_INVALID, "no depth -> cloud call yet");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, (const char *)c->cloud_fws + 64, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));      // (24 words behind the 16 state words)
    return TDLO_OK;
}

int tdlo_debug_exp2(tdlo_ctx *c, const double *x, double *y, int n) {
    if (!c || !x || !y || n < 1) return TDLO_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    double *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, 2 * (size_t)n * sizeof(double)));
    hipError_t e = hipMemcpyAsync(d, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_debug_exp2(d, d + n, n, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(y, d + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(d);
    HIPCHK(c, e);
    return TDLO_OK;
}

// ---- host helpers --------------------------------------------------------------------------------
int tdlo_calc_lle_weights(int k, const double *Y, int M, double *L) {
    if (!Y || !L || M < 1 || k < 2 || k > 13) return TDLO_E_INVALID;
    lle_weights(k, Y, M, L);
    return TDLO_OK;
}

int tdlo_calc_lle_regulariser(const double *Y, int M, double *H, double *Hb) {
    if (!Y || M < 1 || (!H && !Hb)) return TDLO_E_INVALID;
    if (H) {
        std::vector<double> L((size_t)M * M);
        lle_weights(6, Y, M, L.data());
        lle_regulariser(L.data(), M, H);
    }
    if (Hb) lle_regulariser_band(Y, M, Hb);
    return TDLO_OK;
}

int tdlo_line_sphere_intersection(const double A[3], const double B[3], const double C[3], double radius, double out[6]) {
    Vec3 o[2];
    const int n = line_sphere(Vec3{A[0], A[1], A[2]}, Vec3{B[0], B[1], B[2]}, Vec3{C[0], C[1], C[2]}, radius, o);
    for (int i = 0; i < n; ++i) { out[3 * i] = o[i].x; out[3 * i + 1] = o[i].y; out[3 * i + 2] = o[i].z; }
    return n;
}

double tdlo_piecewise_error(const double *Y_track, int n_track, const double *Y_true, int n_true) {
    if (!Y_track || !Y_true || n_track < 1 || n_true < 2) return -1.0;
    return piecewise_error(Y_track, n_track, Y_true, n_true);
}

double tdlo_compute_error(const double *Y_track, int n_track, const double *Y_true, int n_true) {
    if (!Y_track || !Y_true || n_track < 2 || n_true < 2) return -1.0;
    return 0.5 * (piecewise_error(Y_track, n_track, Y_true, n_true) + piecewise_error(Y_true, n_true, Y_track, n_track));
}

int tdlo_traverse_euclidean(const double *coord, int n_coord, const double *guide, int Mg, const int *vis, int n_vis,
                            int alignment, int anchor, double *out) {
    if (!coord || !guide || !vis || !out) return TDLO_E_INVALID;
    std::vector<double> cv(coord, coord + n_coord), res;
    std::vector<int> vv(vis, vis + n_vis);
    const int n = traverse_euclidean(cv, guide, Mg, vv, alignment, anchor, res);
    if (n < 0) return TDLO_E_TRAVERSE;
    std::memcpy(out, res.data(), sizeof(double) * res.size());
    return n;
}

}  // extern "C"

// =================================================================================================
// class trackdlo (trackdlo/include/trackdlo.h:53-130)
// =================================================================================================
struct tdlo_tracker {
    tdlo_ctx *ctx;
    int slot;
    int M;
    int precision = TDLO_PREC_F32;
    // members of the reference class, trackdlo.h:104-121
    std::vector<double> Y;              // M x 3 column-major
    std::vector<double> guide_nodes;    // Mg x 3 column-major
    int Mg;
    double sigma2, beta, beta_pre_proc, lambda, lambda_pre_proc, alpha, k_vis, mu, tol, lle_weight;
    int max_iter;
    std::vector<double> geodesic_coord;
    std::vector<double> priors;         // K x 4 row-major
    double visibility_threshold;
    std::vector<double> trav1, trav2, trav2r;      // scratch of the priors' formation, kept across frames (their growth was a dozen reallocations per frame,
    std::vector<int> vis_ext;                      // on the host path between the two registrations)
    std::vector<int> frame_vis, frame_vis_ext;     // tdlo_tracker_frame_from_depth: the frame's visible sets
    std::vector<double> frame_dist;                // ... and the nodes' distances to the frame's cloud
    bool painter_on = false;                       // tdlo_tracker_set_self_occlusion: frame_from_depth applies trackdlo_node.cpp:279-343 (off by default)
    double painter_proj[12] = {0};
    int painter_width = 0;
    int rig_painter_K = 0;                         // tdlo_tracker_set_rig_self_occlusion: the rig frame calls apply the test under a rig (0: off, the default)
    std::vector<double> rig_painter_T;             // ... its K x 12 rig_to_cam entries, copied (empty: every camera frame is the rig frame)
    int rig_painter_width = 0;
    // tdlo_tracker_render_result: the nodes the last frame_from_* call STARTED from (kept only while the self-occlusion test is on: the picture's
    // not-self-occluded set is formed from them, trackdlo_node.cpp:279-343 / :401) and that call's intrinsics
    std::vector<double> frame_Y0;
    double frame_cam[4] = {0, 0, 0, 0};
    bool frame_seen = false;
    int last_iters[2] = {0, 0};         // iterations the two registrations of the previous frame took: how many are enqueued before the host looks (tdlo_ctx::iter_hint;
                                        // the larger of the last two frames' counts was tried instead: no difference)
};

extern "C" {

tdlo_tracker *tdlo_tracker_create(tdlo_ctx *ctx, int slot, int M, double visibility_threshold, double beta, double lambda,
                                  double alpha, double k_vis, double mu, int max_iter, double tol, double beta_pre_proc,
                                  double lambda_pre_proc, double lle_weight) {
    if (!ctx || slot < 0 || slot >= (int)ctx->slots.size() || M < 1) return nullptr;
    tdlo_tracker *t = new tdlo_tracker();
    t->ctx = ctx; t->slot = slot; t->M = M;
    t->Y.assign(3 * (size_t)M, 0.0);                       // trackdlo.cpp:43
    t->guide_nodes = t->Y; t->Mg = M;                      // :45
    t->sigma2 = 0.0;                                       // :46
    t->visibility_threshold = visibility_threshold; t->beta = beta; t->beta_pre_proc = beta_pre_proc;
    t->lambda = lambda; t->lambda_pre_proc = lambda_pre_proc; t->alpha = alpha; t->lle_weight = lle_weight;
    t->k_vis = k_vis; t->mu = mu; t->max_iter = max_iter; t->tol = tol;
    return t;
}

tdlo_tracker *tdlo_tracker_create_default(tdlo_ctx *ctx, int slot, int M) {
    // trackdlo.cpp:10-28
    return tdlo_tracker_create(ctx, slot, M, /*visibility_threshold*/ 0.02, /*beta*/ 5.0, /*lambda*/ 1.0, /*alpha*/ 0.0,
                               /*k_vis*/ 0.0, /*mu*/ 0.05, /*max_iter*/ 50, /*tol*/ 0.00001, /*beta_pre_proc*/ 3.0,
                               /*lambda_pre_proc*/ 1.0, /*lle_weight*/ 1.0);
}

void tdlo_tracker_destroy(tdlo_tracker *t) { g_prof.report(); delete t; }

int tdlo_tracker_set_precision(tdlo_tracker *t, int precision) {
    if (!t || (precision != TDLO_PREC_F32 && precision != TDLO_PREC_F64)) return TDLO_E_INVALID;
    t->precision = precision;
    return TDLO_OK;
}

int tdlo_tracker_initialize_nodes(tdlo_tracker *t, const double *Y_init) {
    if (!t || !Y_init) return TDLO_E_INVALID;
    t->Y.assign(Y_init, Y_init + 3 * (size_t)t->M);
    t->guide_nodes = t->Y; t->Mg = t->M;
    return TDLO_OK;
}

int tdlo_tracker_initialize_geodesic_coord(tdlo_tracker *t, const double *coord, int n) {
    if (!t || !coord || n < 0) return TDLO_E_INVALID;
    t->geodesic_coord.insert(t->geodesic_coord.end(), coord, coord + n);
    return TDLO_OK;
}

// tdlo_tracker_initialize_from_cloud / _view: reg with M = the tracker's node count on the cloud X, the view v, or -- both null -- what is resident in the
// slot, k_sort_pts behind it on reg's device nodes, one wait, one read-back; the tracker is touched only when everything has succeeded
static int initialize_from_cloud_enqueued(tdlo_tracker *t, const double *X, const tdlo_cloud_view *v, int N, double mu, int max_iter, double *sigma2_out) {
    tdlo_ctx *c = t->ctx;
    const int M = t->M;
    Slot &s = c->slots[t->slot];
    int rc = TDLO_OK;
    if (X) rc = set_cloud_impl(c, t->slot, X, N, false);                 // (X stays the caller's until this call returns: the wait below, or the caller's on an error)
    else if (v) {
        bool device = false;
        if ((rc = view_location(c, v, &device))) return rc;
        rc = import_view(c, t->slot, v, N, device, false);
    }
    else if ((rc = flush_pending_cloud(c))) return rc;
    else if (s.N0 <= 0) rc = fail(c, TDLO_E_INVALID, "X is NULL and no cloud is resident in the tracker's slot");
    if (rc) return rc;
    const size_t nout = sort_pts_out_doubles(M);
    double *out_dev = nullptr;
    if ((rc = reg_enqueue(c, s, M, mu, max_iter, nout, &out_dev))) return rc;
    double *h = c->pin, *ho = h + 8 + 3 * (size_t)M;
    double sigma2;
    std::vector<double> Ys(3 * (size_t)M), coord(M);
    if (!c->init_sort_host) {
        HIPCHK(c, launch_sort_pts(c->reg_ws + 8, c->reg_ws, M, out_dev, c->stream));
        HIPCHK(c, hipMemcpyAsync(ho, out_dev, sizeof(double) * nout, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ++c->init_route[0];
        if (ho[1] != 0.0) return fail(c, TDLO_E_NUMERIC, sort_pts_reason((int)ho[1]));
        sigma2 = ho[0];
        std::memcpy(Ys.data(), ho + 2, sizeof(double) * 3 * (size_t)M);
        std::memcpy(coord.data(), ho + 2 + 3 * (size_t)M, sizeof(double) * M);
    } else {
        HIPCHK(c, hipMemcpyAsync(h, c->reg_ws, sizeof(double) * (8 + 3 * (size_t)M), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ++c->init_route[1];
        if (const int status = sort_pts_host(h + 8, M, Ys.data(), nullptr, coord.data())) return fail(c, TDLO_E_NUMERIC, sort_pts_reason(status));
        sigma2 = h[0];
    }
    t->Y = Ys;                                                           // as tdlo_tracker_initialize_nodes
    t->guide_nodes = t->Y; t->Mg = M;
    t->geodesic_coord = coord;                                           // replaced, not appended to
    if (sigma2_out) *sigma2_out = sigma2;
    return TDLO_OK;
}

static int initialize_from_cloud_impl(tdlo_tracker *t, const double *X, const tdlo_cloud_view *v, int N, double mu, int max_iter, double *sigma2_out) {
    tdlo_ctx *c = t->ctx;
    if (t->M < 4) return fail(c, TDLO_E_INVALID, "initialize_from_cloud: a tracker has at least 4 nodes");
    if (t->M > reg_max_nodes()) return fail(c, TDLO_E_INVALID, "initialize_from_cloud: reg fits at most " + std::to_string(reg_max_nodes()) + " centroids (tdlo_reg)");
    if (max_iter < 0 || !(mu >= 0 && mu < 1)) return fail(c, TDLO_E_INVALID, "initialize_from_cloud: bad reg arguments");
    if (X && N <= 0) return fail(c, TDLO_E_INVALID, "empty cloud");
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = initialize_from_cloud_enqueued(t, X, v, N, mu, max_iter, sigma2_out);
    if (rc && rc != TDLO_E_NUMERIC) (void)hipStreamSynchronize(c->stream);      // nothing of this call stays enqueued behind an error (X and v are the caller's again)
    return rc;
}

int tdlo_tracker_initialize_from_cloud(tdlo_tracker *t, const double *X, int N, double mu, int max_iter, double *sigma2_out) {
    if (!t) return TDLO_E_INVALID;
    return initialize_from_cloud_impl(t, X, nullptr, N, mu, max_iter, sigma2_out);
}

int tdlo_tracker_initialize_from_cloud_view(tdlo_tracker *t, const tdlo_cloud_view *v, int N, double mu, int max_iter, double *sigma2_out) {
    if (!t) return TDLO_E_INVALID;
    if (const char *why = view_fault(v, N)) return fail(t->ctx, TDLO_E_INVALID, why);
    return initialize_from_cloud_impl(t, nullptr, v, N, mu, max_iter, sigma2_out);
}

// tdlo_tracker_initialize_from_cloud for F trackers on the clouds resident in their slots: reg's loops share their launches (reg_batch_enqueue), one
// k_sort_pts_batch launch orders every frame's centroids where reg left them, one read-back, one wait.  A frame is installed exactly as
// initialize_from_cloud_enqueued installs it, or -- its verdict non-zero -- not touched at all.
int tdlo_tracker_initialize_from_cloud_batch(tdlo_tracker *const *trackers, int F, double mu, int max_iter, double *sigma2_out, int *rc_each) {
    if (!trackers || F < 1 || !trackers[0]) return TDLO_E_INVALID;
    tdlo_ctx *c = trackers[0]->ctx;
    const int M = trackers[0]->M;
    std::vector<int> slots(F);
    for (int i = 0; i < F; ++i) {
        const tdlo_tracker *t = trackers[i];
        if (!t) return fail(c, TDLO_E_INVALID, "initialize_from_cloud_batch: a tracker is null");
        if (t->ctx != c) return fail(c, TDLO_E_INVALID, "initialize_from_cloud_batch: the trackers of a batch share one context");
        if (t->M != M) return fail(c, TDLO_E_INVALID, "initialize_from_cloud_batch: the trackers of a batch share num_of_nodes");
        slots[i] = t->slot;
    }
    if (M < 4) return fail(c, TDLO_E_INVALID, "initialize_from_cloud_batch: a tracker has at least 4 nodes");
    if (M > reg_max_nodes()) return fail(c, TDLO_E_INVALID, "initialize_from_cloud_batch: reg fits at most " + std::to_string(reg_max_nodes()) + " centroids (tdlo_reg)");
    if (max_iter < 0 || !(mu >= 0 && mu < 1)) return fail(c, TDLO_E_INVALID, "initialize_from_cloud_batch: bad reg arguments");
    if (const char *why = batch_slots_refusal(c, slots.data(), F)) return fail(c, TDLO_E_INVALID, std::string("initialize_from_cloud_batch: ") + why + " (the trackers' slots)");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int> rcs(F, 0);
    std::string why;
    int first = -1;
    auto failed = [&](int i, int code, const std::string &text) {
        rcs[i] = code;
        if (first < 0) { first = i; why = text; }
    };
    auto finish = [&]() {
        if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
        if (first >= 0) return fail(c, rcs[first], "initialize_from_cloud_batch: frame " + std::to_string(first) + ": " + why);
        return (int)TDLO_OK;
    };
    int rc;
    if (F < init_batch_min(c)) {
        for (int i = 0; i < F; ++i) {
            rc = initialize_from_cloud_impl(trackers[i], nullptr, nullptr, 0, mu, max_iter, sigma2_out ? sigma2_out + i : nullptr);
            if (rc && rc != TDLO_E_NUMERIC) return rc;
            if (rc) failed(i, rc, c->err);
            ++c->ibat_route[1];
        }
        return finish();
    }
    auto enqueued = [&]() -> int {
        if ((rc = flush_pending_cloud(c))) return rc;
        RegBatchRun run;
        if ((rc = reg_batch_enqueue(c, slots.data(), F, M, mu, max_iter, run))) return rc;
        const size_t YM = 3 * (size_t)M;
        std::vector<double> Ys(YM), coord(M);
        if (!c->init_sort_host) {
            HIPCHK(c, launch_sort_pts_batch(run.states_dev + 8, run.S, true, F, M, run.outs_dev, run.O, c->stream));
            HIPCHK(c, hipMemcpyAsync(run.readback, run.outs_dev, sizeof(double) * (size_t)run.O * F, hipMemcpyDeviceToHost, c->stream));
        } else {
            HIPCHK(c, hipMemcpyAsync(run.readback, run.states_dev, sizeof(double) * (size_t)run.S * F, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->ibat_route[0] += F;
        for (int i = 0; i < F; ++i) {
            double sigma2;
            if (!c->init_sort_host) {
                const double *ho = run.readback + (size_t)run.O * i;
                if (ho[1] != 0.0) { failed(i, TDLO_E_NUMERIC, sort_pts_reason((int)ho[1])); continue; }
                sigma2 = ho[0];
                std::memcpy(Ys.data(), ho + 2, sizeof(double) * YM);
                std::memcpy(coord.data(), ho + 2 + YM, sizeof(double) * M);
            } else {
                const double *h = run.readback + (size_t)run.S * i;
                if (const int status = sort_pts_host(h + 8, M, Ys.data(), nullptr, coord.data())) { failed(i, TDLO_E_NUMERIC, sort_pts_reason(status)); continue; }
                sigma2 = h[0];
            }
            tdlo_tracker *t = trackers[i];
            t->Y = Ys;                                                       // as initialize_from_cloud_enqueued
            t->guide_nodes = t->Y; t->Mg = M;
            t->geodesic_coord = coord;                                       // replaced, not appended to
            if (sigma2_out) sigma2_out[i] = sigma2;
        }
        return TDLO_OK;
    };
    if ((rc = enqueued())) { (void)hipStreamSynchronize(c->stream); return rc; }      // nothing of this call stays enqueued behind an error
    return finish();
}

int tdlo_tracker_copy_state(tdlo_tracker *dst, const tdlo_tracker *src) {
    if (!dst || !src || dst->M != src->M) return TDLO_E_INVALID;
    if (dst == src) return TDLO_OK;
    tdlo_ctx *ctx = dst->ctx; const int slot = dst->slot;
    *dst = *src;                                       // every member of trackdlo.h:104-121 (and the precision switch)
    dst->ctx = ctx; dst->slot = slot;
    return TDLO_OK;
}

double tdlo_tracker_get_sigma2(const tdlo_tracker *t) { return t ? t->sigma2 : 0.0; }
void tdlo_tracker_set_sigma2(tdlo_tracker *t, double s) { if (t) t->sigma2 = s; }

int tdlo_tracker_get_tracking_result(const tdlo_tracker *t, double *out) {
    if (!t || !out) return TDLO_E_INVALID;
    std::memcpy(out, t->Y.data(), sizeof(double) * t->Y.size());
    return t->M;
}

int tdlo_tracker_get_guide_nodes(const tdlo_tracker *t, double *out, int max_rows) {
    if (!t || !out) return TDLO_E_INVALID;
    if (max_rows < t->Mg) return TDLO_E_INVALID;
    std::memcpy(out, t->guide_nodes.data(), sizeof(double) * 3 * (size_t)t->Mg);
    return t->Mg;
}

int tdlo_tracker_get_correspondence_pairs(const tdlo_tracker *t, double *out, int max_rows) {
    if (!t || !out) return TDLO_E_INVALID;
    const int K = (int)(t->priors.size() / 4);
    if (max_rows < K) return TDLO_E_INVALID;
    std::memcpy(out, t->priors.data(), sizeof(double) * t->priors.size());
    return K;
}

// The priors of tracking_step's main registration (trackdlo.cpp:929-995), formed from the pre-processing registration's result in t->guide_nodes for the
// visible nodes in t->vis_ext; vis / n_vis: the frame's visible_nodes (the anchor search of :980-995).  Appends to / replaces t->priors as the reference does.
static int tracker_form_priors(tdlo_tracker *t, const int *vis, int n_vis) {
    tdlo_ctx *c = t->ctx;
    const int M = t->M, Mg = t->Mg;
    std::vector<int> &ve = t->vis_ext;
    std::vector<double> &p1 = t->trav1, &p2 = t->trav2;
    const double *guide = t->guide_nodes.data();
    auto trav = [&](int alignment, int anchor, std::vector<double> &out) {
        return traverse_euclidean(t->geodesic_coord, guide, Mg, ve, alignment, anchor, out);
    };
    const char *oob = "traverse_euclidean: the reference would index out of bounds for these visible nodes";
    if (Mg == M) {                                                       // all visible / minor occlusion (:929-957)
        const int n1 = trav(0, -1, p1), n2 = trav(1, -1, p2);
        if (n1 <= 0 || n2 <= 0) return fail(c, TDLO_E_TRAVERSE, oob);
        // p2 runs tail -> head; bring it to ascending order (:942)
        std::vector<double> &r2 = t->trav2r;
        r2.resize(p2.size());
        for (int i = 0; i < n2; ++i) std::memcpy(&r2[4 * i], &p2[4 * (n2 - 1 - i)], 4 * sizeof(double));
        t->priors.reserve(t->priors.size() + 4 * (size_t)M);
        for (int i = 0; i < M; ++i) {
            const long long j2 = (long long)i - ((long long)M - n2);     // unsigned in the reference: negative == huge
            const bool j2_ok = j2 >= 0 && j2 < n2;
            if ((double)i < r2[0] && i < n1) {
                t->priors.insert(t->priors.end(), &p1[4 * i], &p1[4 * i] + 4);
            } else if ((double)i > p1[4 * (n1 - 1)] && j2_ok) {
                t->priors.insert(t->priors.end(), &r2[4 * j2], &r2[4 * j2] + 4);
            } else {
                if (i >= n1 || !j2_ok) return fail(c, TDLO_E_TRAVERSE, oob);
                for (int k = 0; k < 4; ++k) t->priors.push_back((p1[4 * i + k] + r2[4 * j2 + k]) / 2.0);    // :954
            }
        }
    } else if (ve.front() == 0 && ve.back() == M - 1) {                  // mid-section occluded (:958-967)
        if (trav(0, -1, p1) < 0 || trav(1, -1, p2) < 0) return fail(c, TDLO_E_TRAVERSE, oob);
        t->priors = p1;
        t->priors.insert(t->priors.end(), p2.begin(), p2.end());
    } else if (ve.front() == 0) {                                        // tail occluded (:968-973)
        if (trav(0, -1, p1) < 0) return fail(c, TDLO_E_TRAVERSE, oob);
        t->priors = p1;
    } else if (ve.back() == M - 1) {                                     // head occluded (:974-979)
        if (trav(1, -1, p1) < 0) return fail(c, TDLO_E_TRAVERSE, oob);
        t->priors = p1;
    } else {                                                             // both ends occluded (:980-995)
        int anchor = -1; double moved = 999999;
        for (int i = 0; i < n_vis && i < Mg; ++i) {                      // reference pairs visible_nodes[i] with guide row i
            double s = 0;
            for (int d = 0; d < 3; ++d) { const double e = t->Y[d * M + vis[i]] - t->guide_nodes[d * Mg + i]; s += e * e; }
            const double dd = std::sqrt(s);
            if (dd < moved) { moved = dd; anchor = i; }
        }
        if (trav(2, anchor, p1) < 0) return fail(c, TDLO_E_TRAVERSE, oob);
        t->priors = p1;
    }
    return 0;
}

// tdlo_tracker_tracking_step / _view: the frame's cloud is X (N x 3 column-major doubles), the view v, or -- both null -- what is resident in the slot
static int tracking_step_impl(tdlo_tracker *t, const double *X, const tdlo_cloud_view *v, int N, const int *vis, int n_vis,
                              const int *vis_ext, int n_ext, const double *H_pre, tdlo_stats *stats) {
    if (!t || !vis_ext) return TDLO_E_INVALID;
    tdlo_ctx *c = t->ctx;
    const int M = t->M;
    if (n_ext <= 0 || n_ext > M) return fail(c, TDLO_E_INVALID, "visible_nodes_extended must hold 1..M indices (empty is undefined in the reference, trackdlo_node.cpp:351)");
    for (int i = 0; i < n_ext; ++i) if (vis_ext[i] < 0 || vis_ext[i] >= M) return fail(c, TDLO_E_INVALID, "visible_nodes_extended index out of range");
    for (int i = 0; i < n_vis; ++i) if (vis[i] < 0 || vis[i] >= M) return fail(c, TDLO_E_INVALID, "visible_nodes index out of range");
    t->priors.clear();                                                   // :908
    int rc = TDLO_OK;
    g_prof.start(); g_prof.base = 0;
    bool staged = false;          // this frame's cloud is in the pinned staging buffer
    if (X && N > 0 && c->cloud_direct_on && c->direct_in && c->fuse_on && N <= 16384) {
        // a cloud the fused prologue can take (up to 64 point workgroups): staged in pinned host memory, read from there by the prologue itself
        HIPCHK(c, hipSetDevice(c->device));
        Slot &s = c->slots[t->slot];
        if ((rc = flush_pending_cloud(c)) || (rc = ensure_points(c, s, N)) || (rc = ensure_cloud_pin(c, 3 * (size_t)N))) return rc;
        std::memcpy(c->cloud_pin, X, 3 * (size_t)N * sizeof(double));
        s.N0 = N; s.sorted_valid = false;
        c->cloud_pending = t->slot;
        staged = true;
    }
    else if (X) rc = set_cloud_impl(c, t->slot, X, N, false);            // X_orig by value: one upload for both registrations (X stays the caller's
                                                                         // until this function returns; the first registration's read-back waits for the copy)
    else if (v) {
        HIPCHK(c, hipSetDevice(c->device));
        bool device = false;
        if ((rc = view_location(c, v, &device))) return rc;
        if (!device && c->cloud_direct_on && c->direct_in && c->fuse_on && N <= 16384) {
            // a host view of a small frame: widened straight into the pinned staging, where the memcpy above stands -- the same route from there on
            Slot &s = c->slots[t->slot];
            if ((rc = flush_pending_cloud(c)) || (rc = ensure_points(c, s, N)) || (rc = ensure_cloud_pin(c, 3 * (size_t)N))) return rc;
            if (v->dtype == TDLO_F64) view_gather(c->cloud_pin, (const double *)v->data, v->stride_point, v->stride_comp, N);
            else view_gather(c->cloud_pin, (const float *)v->data, v->stride_point, v->stride_comp, N);
            s.N0 = N; s.sorted_valid = false;
            c->cloud_pending = t->slot;
            staged = true;
            ++c->view_route[1];
        }
        else rc = import_view(c, t->slot, v, N, device, false);         // enqueued: the first registration's read-back waits for it
    }
    else if (c->slots[t->slot].N0 <= 0) rc = fail(c, TDLO_E_INVALID, "X is NULL and no cloud is resident in the tracker's slot");
    if (rc) return rc;
    g_prof.mark(0);

    // guide nodes = visible sub-chain (:913-921)
    const int Mg = n_ext;
    t->Mg = Mg;
    t->guide_nodes.assign(3 * (size_t)Mg, 0.0);
    if (Mg != M) { for (int i = 0; i < Mg; ++i) for (int d = 0; d < 3; ++d) t->guide_nodes[d * Mg + i] = t->Y[d * M + vis_ext[i]]; }
    else t->guide_nodes = t->Y;

    // pre-processing registration (:925-927): sigma2 copy, beta/lambda_pre_proc, include_lle = true
    tdlo_params pp{};
    pp.beta = t->beta_pre_proc; pp.lambda = t->lambda_pre_proc; pp.lle_weight = t->lle_weight; pp.mu = t->mu;
    pp.max_iter = t->max_iter; pp.tol = t->tol; pp.include_lle = 1; pp.alpha = 0; pp.k_vis = 0; pp.visibility_threshold = 0.01;
    pp.precision = t->precision;
    double sigma2_pre = t->sigma2;
    tdlo_stats st_pre{}, st_main{};
    // the main registration's parameters (:998): include_lle = false, priors, alpha, visible_nodes_extended, k_vis
    tdlo_params mp{};
    mp.beta = t->beta; mp.lambda = t->lambda; mp.lle_weight = t->lle_weight; mp.mu = t->mu; mp.max_iter = t->max_iter;
    mp.tol = t->tol; mp.include_lle = 0; mp.alpha = t->alpha; mp.k_vis = t->k_vis; mp.visibility_threshold = t->visibility_threshold;
    mp.precision = t->precision;
    // every node visible: both registrations start from t->Y, and the main one's node-side set-up depends on nothing the pre-processing one
    // produces -- the pre-processing registration's prologue is asked to do it as well (tdlo_ctx::PairNext; run_frames takes it up if it can)
    if (c->lle_next_on && M <= 256 && (rc = ensure_hb_next(c, c->slots[t->slot], M))) return rc;
    c->pair.state = 0; c->pair.ahead = false;
    if (Mg == M && c->pair_on && c->sort_reuse && c->late_on && c->direct_in && c->fuse_on && check_params(c, M, &mp) == 0) {
        tdlo_ctx::PairNext &pn = c->pair;
        pn.slot = t->slot; pn.M = M; pn.n_vis = n_ext; pn.sigma2 = t->sigma2; pn.p = mp; pn.Y = t->Y;
        pn.state = 1;
    } else if (Mg != M && staged && c->ahead_on && c->pair_on && c->late_on && c->direct_in && c->fuse_on && c->spec_on && c->mbox_on && !c->timing && M <= 256 &&
               mp.max_iter > 0 && check_params(c, M, &mp) == 0) {
        // hidden nodes: the registrations start from different node sets, but the main one's prologue, k_dmin and first E-step need nothing the
        // pre-processing one produces -- they are asked to run beside it (PairNext::ahead; the pre-processing registration's run_frames launches
        // them).  What they will point at is sized here, before anything is launched: the larger registration's mailbox and late-priors buffer
        const NodeCarve ncm(M);
        if ((rc = ensure_mbox(c, ncm.readback + 4)) || (rc = ensure_late(c, 4 * (size_t)M + 2))) return rc;
        tdlo_ctx::PairNext &pn = c->pair;
        pn.slot = t->slot; pn.M = M; pn.n_vis = n_ext; pn.sigma2 = t->sigma2; pn.p = mp; pn.Y = t->Y; pn.cloud_in_pin = true;
        pn.state = 3;
    }
    g_prof.mark(1);
    c->iter_hint = t->last_iters[0]; c->iter_hint_next = t->last_iters[1];
    rc = tdlo_cpd_lle_resident(c, t->slot, t->guide_nodes.data(), Mg, &sigma2_pre, &pp, nullptr, 0, nullptr, 0, H_pre, &st_pre);
    t->last_iters[0] = rc ? 0 : st_pre.iters;
    if (stats) stats[0] = st_pre;
    if (rc) {        // (an early error return may not have waited for the cloud's copy yet; what was launched ahead is told to leave and drained)
        c->pair.state = 0; c->pair.ahead = false; c->iter_hint = 0; c->iter_hint_next = 0; spec_abort(c); (void)flush_pending_cloud(c); (void)hipStreamSynchronize(c->stream);
        if (c->twin_busy && c->stream2[0]) { (void)hipStreamSynchronize(c->stream2[0]); c->twin_busy = false; }
        return rc;
    }

    t->vis_ext.assign(vis_ext, vis_ext + n_ext);
    // The priors of the main registration (:929-995), formed from the pre-processing registration's result.  As a function: the main registration's
    // set-up kernel does not need them, so run_frames launches it first and calls this while it runs (LatePriors).
    const LatePriors form_priors = [&](const double *&lp, int &lk) -> int {
        if (const int prc = tracker_form_priors(t, vis, n_vis)) return prc;
        lp = t->priors.data(); lk = (int)(t->priors.size() / 4);
        return 0;
    };

    // main registration (:998): include_lle = false, priors, alpha, visible_nodes_extended, k_vis (mp, above)
    // prior indices may be fractional after the averaging at :954; the reference truncates (:247)
    g_prof.mark(13); g_prof.base = 6;
    HIPCHK(c, hipSetDevice(c->device));
    c->iter_hint = t->last_iters[1];
    rc = run_frames(c, 1, &t->slot, t->Y.data(), M, &t->sigma2, &mp, nullptr, 0, vis_ext, n_ext, nullptr, &st_main, &form_priors);
    if (rc == TDLO_E_FUSE) {
        // the main registration's own fused prologue (hidden nodes: in the slot, or launched ahead in the twin slot) was abandoned: Y_, sigma2_ and the
        // cloud in the slot are untouched -- once more on the three-kernel route, the priors formed again from the same guide nodes
        fuse_fallback(c);
        t->priors.clear();
        rc = run_frames(c, 1, &t->slot, t->Y.data(), M, &t->sigma2, &mp, nullptr, 0, vis_ext, n_ext, nullptr, &st_main, &form_priors);
        if (rc == TDLO_E_FUSE) rc = fail(c, TDLO_E_HIP, "the fused prologue reported a time-out on the route that does not use it");
    }
    t->last_iters[1] = rc ? 0 : st_main.iters;
    c->iter_hint = 0; c->iter_hint_next = 0;
    c->pair.state = 0; c->pair.ahead = false; spec_abort(c);
    if (c->cloud_pending >= 0) { const int frc = flush_pending_cloud(c); if (!rc) rc = frc; }
    if (stats) stats[1] = st_main;
    return rc;
}

int tdlo_tracker_tracking_step(tdlo_tracker *t, const double *X, int N, const int *vis, int n_vis,
                               const int *vis_ext, int n_ext, const double *H_pre, tdlo_stats *stats) {
    return tracking_step_impl(t, X, nullptr, N, vis, n_vis, vis_ext, n_ext, H_pre, stats);
}

int tdlo_tracker_tracking_step_view(tdlo_tracker *t, const tdlo_cloud_view *v, int N, const int *vis, int n_vis,
                                    const int *vis_ext, int n_ext, const double *H_pre, tdlo_stats *stats) {
    if (!t) return TDLO_E_INVALID;
    if (const char *why = view_fault(v, N)) return fail(t->ctx, TDLO_E_INVALID, why);
    return tracking_step_impl(t, nullptr, v, N, vis, n_vis, vis_ext, n_ext, H_pre, stats);
}

// One frame of the ROS node's callback, images in, nodes out (trackdlo_node.cpp:195-369): depth image + mask -> cloud -> voxel grid and the visibility
// pre-pass of the tracker's nodes (tdlo_depth_to_cloud_visibility: one launch), then tracking_step on the cloud resident in the tracker's slot.
static int tracker_frame_impl(tdlo_tracker *t, const unsigned short *depth, const unsigned char *mask, const ColourIn *colour, int rows, int cols,
                              double fx, double fy, double cx, double cy, double leaf_size, double d_vis,
                              int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                              int *n_out, int *n_raw_out, tdlo_stats *stats) {
    if (!t) return TDLO_E_INVALID;
    tdlo_ctx *c = t->ctx;
    const int M = t->M;
    if (t->geodesic_coord.size() != (size_t)M) return fail(c, TDLO_E_INVALID, "the tracker has no nodes / geodesic coordinates yet (tdlo_tracker_initialize_*)");
    std::vector<int> &ve = t->frame_vis_ext, &v = t->frame_vis;
    v.resize(M); ve.resize(M);
    int nv = 0, ne = 0, n = 0;
    t->frame_dist.resize(M);
    t->frame_cam[0] = fx; t->frame_cam[1] = fy; t->frame_cam[2] = cx; t->frame_cam[3] = cy; t->frame_seen = true;
    if (t->painter_on) t->frame_Y0 = t->Y; else t->frame_Y0.clear();
    int rc = depth_to_cloud_visibility_impl(c, t->slot, depth, mask, colour, rows, cols, fx, fy, cx, cy, leaf_size, t->Y.data(), M, t->visibility_threshold, d_vis,
                                            t->geodesic_coord.data(), t->frame_dist.data(), v.data(), &nv, ve.data(), &ne, &n, n_raw_out);
    if (!rc && t->painter_on && n > 0) {
        // the callback's self-occlusion test (trackdlo_node.cpp:279-343) between the distance pre-pass and the gap fill, when the tracker was given a
        // projection matrix for it (tdlo_tracker_set_self_occlusion; off by default: parity against OpenCV's rasteriser is unpinned)
        std::vector<int> pv, pe;
        self_occlusion_visible(t->Y.data(), M, t->painter_proj, t->painter_width, t->frame_dist.data(), t->visibility_threshold, pv);
        fill_visible_gaps(pv, t->geodesic_coord.data(), d_vis, pe);
        nv = (int)pv.size(); ne = (int)pe.size();
        std::copy(pv.begin(), pv.end(), v.begin()); std::copy(pe.begin(), pe.end(), ve.begin());
    }
    if (n_out) *n_out = n;
    if (n_vis) *n_vis = nv;
    if (n_vis_ext) *n_vis_ext = ne;
    if (visible_nodes) std::copy(v.begin(), v.begin() + nv, visible_nodes);
    if (visible_nodes_extended) std::copy(ve.begin(), ve.begin() + ne, visible_nodes_extended);
    if (rc) return rc;
    // (the reference's callback indexes visible_nodes[size() - 1] without a test, trackdlo_node.cpp:351-361: a frame without a cloud or without a visible node is an error here)
    if (n == 0) return fail(c, TDLO_E_EMPTY, "the mask selects no pixel: no cloud for this frame");
    if (ne == 0) return fail(c, TDLO_E_EMPTY, "no node within the visibility threshold of the cloud (the reference's callback is undefined here, trackdlo_node.cpp:351)");
    return tdlo_tracker_tracking_step(t, nullptr, 0, v.data(), nv, ve.data(), ne, nullptr, stats);
}

int tdlo_tracker_frame_from_depth(tdlo_tracker *t, const unsigned short *depth, const unsigned char *mask, int rows, int cols,
                                  double fx, double fy, double cx, double cy, double leaf_size, double d_vis,
                                  int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                  int *n_out, int *n_raw_out, tdlo_stats *stats) {
    return tracker_frame_impl(t, depth, mask, nullptr, rows, cols, fx, fy, cx, cy, leaf_size, d_vis, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext,
                              n_out, n_raw_out, stats);
}

// The same from the two sensor images (trackdlo_node.cpp:158-277, :345-369): the segmentation is formed from the colour image on the device
int tdlo_tracker_frame_from_colour(tdlo_tracker *t, const unsigned short *depth, const unsigned char *colour, const tdlo_colour_params *params,
                                   const unsigned char *occluder, int rows, int cols,
                                   double fx, double fy, double cx, double cy, double leaf_size, double d_vis,
                                   int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                   int *n_out, int *n_raw_out, tdlo_stats *stats) {
    const ColourIn ci{colour, params, occluder};
    return tracker_frame_impl(t, depth, nullptr, &ci, rows, cols, fx, fy, cx, cy, leaf_size, d_vis, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext,
                              n_out, n_raw_out, stats);
}

// The same from views of the images where they lie (tdlo_image_view): refused before the tracker's state is touched, staged, then the packed route
int tdlo_tracker_frame_view(tdlo_tracker *t, const tdlo_frame_view *fv, const tdlo_colour_params *colour_params, int rows, int cols,
                            double fx, double fy, double cx, double cy, double leaf_size, double d_vis,
                            int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                            int *n_out, int *n_raw_out, tdlo_stats *stats) {
    if (!t) return TDLO_E_INVALID;
    tdlo_ctx *c = t->ctx;
    if (t->geodesic_coord.size() != (size_t)t->M) return fail(c, TDLO_E_INVALID, "the tracker has no nodes / geodesic coordinates yet (tdlo_tracker_initialize_*)");
    int rc = frame_view_refusal(c, t->slot, fv, colour_params, rows, cols, fx, fy, leaf_size);
    if (rc) return rc;
    StagedFrame sf;
    if ((rc = stage_frame_view(c, fv, colour_params, rows, cols, sf))) return rc;
    return tracker_frame_impl(t, sf.depth, sf.mask, sf.colour ? &sf.ci : nullptr, rows, cols, fx, fy, cx, cy, leaf_size, d_vis, visible_nodes, n_vis,
                              visible_nodes_extended, n_vis_ext, n_out, n_raw_out, stats);
}

// tdlo_tracker_frame_view on two raw streams: the align launches in front of the import, on the same stream -- no host wait of their own
int tdlo_tracker_frame_view_aligning(tdlo_tracker *t, const tdlo_frame_view *fv, const tdlo_align_params *p, const tdlo_colour_params *colour_params,
                                     double leaf_size, double d_vis,
                                     int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                     int *n_out, int *n_raw_out, tdlo_stats *stats, long long counts[4]) {
    if (!t) return TDLO_E_INVALID;
    tdlo_ctx *c = t->ctx;
    if (t->geodesic_coord.size() != (size_t)t->M) return fail(c, TDLO_E_INVALID, "the tracker has no nodes / geodesic coordinates yet (tdlo_tracker_initialize_*)");
    tdlo_frame_view fv2;
    bool dev = false;
    int rc = align_frame_refusal(c, t->slot, fv, p, colour_params, leaf_size, fv2, &dev);
    if (rc) return rc;
    const unsigned short *plane = nullptr;
    StagedFrame sf;
    if ((rc = align_enqueue(c, &fv->depth, dev, p, &plane)) || (fv2.depth.data = plane, rc = stage_frame_view(c, &fv2, colour_params, p->rows_c, p->cols_c, sf))) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    rc = tracker_frame_impl(t, sf.depth, sf.mask, sf.colour ? &sf.ci : nullptr, p->rows_c, p->cols_c, p->fx_c, p->fy_c, p->cx_c, p->cy_c, leaf_size, d_vis,
                            visible_nodes, n_vis, visible_nodes_extended, n_vis_ext, n_out, n_raw_out, stats);
    if (rc) (void)hipStreamSynchronize(c->stream);
    align_counts_fetch(c, counts);
    return rc;
}

// The same from a cloud view: the voxel grid on the view into the tracker's slot and the visibility pre-pass (tdlo_cloud_view_voxel_grid_visibility: in one
// launch where the team kernel serves the view), tdlo_tracker_tracking_step -- the bits of the three calls made by hand
int tdlo_tracker_frame_from_cloud_view(tdlo_tracker *t, const tdlo_cloud_view *v, int N, const unsigned char *select, double leaf_size, double d_vis,
                                       int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                       int *n_out, int *n_raw_out, tdlo_stats *stats) {
    if (!t) return TDLO_E_INVALID;
    tdlo_ctx *c = t->ctx;
    const int M = t->M;
    if (t->geodesic_coord.size() != (size_t)M) return fail(c, TDLO_E_INVALID, "the tracker has no nodes / geodesic coordinates yet (tdlo_tracker_initialize_*)");
    int rc = voxel_view_refusal(c, t->slot, v, N, leaf_size);
    if (rc) return rc;
    std::vector<int> &ve = t->frame_vis_ext, &vv = t->frame_vis;
    vv.resize(M); ve.resize(M);
    int nv = 0, ne = 0, n = 0;
    t->frame_dist.resize(M);
    if (t->painter_on) t->frame_Y0 = t->Y; else t->frame_Y0.clear();
    rc = tdlo_cloud_view_voxel_grid_visibility(c, t->slot, v, N, select, leaf_size, t->Y.data(), M, t->visibility_threshold, d_vis, t->geodesic_coord.data(),
                                               t->frame_dist.data(), vv.data(), &nv, ve.data(), &ne, &n, n_raw_out);
    if (!rc && t->painter_on && n > 0) {      // the self-occlusion switch, as in tracker_frame_impl
        std::vector<int> pv, pe;
        self_occlusion_visible(t->Y.data(), M, t->painter_proj, t->painter_width, t->frame_dist.data(), t->visibility_threshold, pv);
        fill_visible_gaps(pv, t->geodesic_coord.data(), d_vis, pe);
        nv = (int)pv.size(); ne = (int)pe.size();
        std::copy(pv.begin(), pv.end(), vv.begin()); std::copy(pe.begin(), pe.end(), ve.begin());
    }
    if (n_out) *n_out = n;
    if (n_vis) *n_vis = nv;
    if (n_vis_ext) *n_vis_ext = ne;
    if (visible_nodes) std::copy(vv.begin(), vv.begin() + nv, visible_nodes);
    if (visible_nodes_extended) std::copy(ve.begin(), ve.begin() + ne, visible_nodes_extended);
    if (rc) return rc;
    if (n == 0) return fail(c, TDLO_E_EMPTY, "no point of the view is kept: no cloud for this frame");
    if (ne == 0) return fail(c, TDLO_E_EMPTY, "no node within the visibility threshold of the cloud (the reference's callback is undefined here, trackdlo_node.cpp:351)");
    return tdlo_tracker_tracking_step(t, nullptr, 0, vv.data(), nv, ve.data(), ne, nullptr, stats);
}

// ---- self-occlusion under a rig (include/trackdlo_hip.h has the statement; tdlo_painter_lane.h the lane, tdlo_painter_host.cpp the host statement) ----
// From this many (camera, frame) jobs on, the rig tracker calls hand the test to k_rig_painter_batch; below it they run the host statement: the same sets.
// NOT MEASURED YET (scripts/gpu_rig_painter.py writes profiles/rig_painter_ab.txt; the rule: the smallest F K from which the kernel wins on every measured value
// at M = 45 and M = 300, else a value above any batch): until it is, the default is the host statement.  TDLO_RIG_PAINTER_MIN=n, read when the context is
// made, overrides.
constexpr int kRigPainterMin = 1 << 30;
static int rig_painter_min(const tdlo_ctx *c) { return c->rig_painter_min ? c->rig_painter_min : kRigPainterMin; }

// where the kernel's words of the frames of one call lie in pnt_pin (valid until the next enqueue)
struct PainterWords { std::vector<const unsigned *> seen, hidden; };

// One upload of [frame table | camera records | nodes], one launch; the words are in place once the stream has passed the launch.  The frames are checked
// (rig_painter_fault); nothing waits here
static int rig_painter_enqueue(tdlo_ctx *c, int F, const tdlo_rig_painter_frame *fr, int rows, int cols, PainterWords &pw) {
    HIPCHK(c, hipSetDevice(c->device));
    size_t sumK = 0, sumY = 0, sumW = 0;
    int Kmax = 0;
    for (int f = 0; f < F; ++f) {
        sumK += (size_t)fr[f].K; sumY += 3 * (size_t)fr[f].M; sumW += (size_t)fr[f].K * ((fr[f].M + 31) / 32);
        Kmax = std::max(Kmax, fr[f].K);
    }
    const size_t cams_off = sizeof(PainterFrame) * (size_t)F, y_off = cams_off + sizeof(PainterCam) * sumK, up = y_off + sizeof(double) * sumY;
    const size_t pin_bytes = up + sizeof(unsigned) * 2 * sumW;
    hipStream_t st = c->stream;
    if (up > c->pnt_dev_cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->pnt_dev) hipFree(c->pnt_dev);
        c->pnt_dev = nullptr; c->pnt_dev_cap = 0;
        const size_t cap = (up + (up >> 1) + 4095) & ~(size_t)4095;
        HIPCHK(c, hipMalloc(&c->pnt_dev, cap));
        c->pnt_dev_cap = cap;
    }
    if (pin_bytes > c->pnt_pin_cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->pnt_pin) hipHostFree(c->pnt_pin);
        c->pnt_pin = nullptr; c->pnt_pin_cap = 0;
        const size_t cap = (pin_bytes + (pin_bytes >> 1) + 4095) & ~(size_t)4095;
        HIPCHK(c, hipHostMalloc((void **)&c->pnt_pin, cap, hipHostMallocDefault));
        std::memset(c->pnt_pin, 0, cap);
        c->pnt_pin_cap = cap;
    }
    char *pin = c->pnt_pin, *dev = (char *)c->pnt_dev;
    PainterFrame *tab = (PainterFrame *)pin;
    PainterCam *cams = (PainterCam *)(pin + cams_off);
    double *Yp = (double *)(pin + y_off);
    unsigned *words = (unsigned *)(pin + up);
    pw.seen.assign(F, nullptr); pw.hidden.assign(F, nullptr);
    size_t ik = 0, iy = 0, iw = 0;
    for (int f = 0; f < F; ++f) {
        const int M = fr[f].M, K = fr[f].K, W = (M + 31) / 32;
        for (int k = 0; k < K; ++k) rig_painter_camera(fr[f].cams[k], fr[f].rig_to_cam ? fr[f].rig_to_cam + 12 * (size_t)k : nullptr, cams[ik + k]);
        std::memcpy(Yp + iy, fr[f].Y, sizeof(double) * 3 * M);
        tab[f] = PainterFrame{(const double *)(dev + y_off) + iy, (const PainterCam *)(dev + cams_off) + ik, words + iw, words + iw + (size_t)K * W, M, K, fr[f].dlo_pixel_width, 0};
        pw.seen[f] = words + iw; pw.hidden[f] = words + iw + (size_t)K * W;
        ik += (size_t)K; iy += 3 * (size_t)M; iw += 2 * (size_t)K * W;
    }
    HIPCHK(c, hipMemcpyAsync(dev, pin, up, hipMemcpyHostToDevice, st));
    HIPCHK(c, launch_rig_painter_batch((const PainterFrame *)dev, F, Kmax, rows, cols, st));
    c->pnt_route[0] += (long long)sumK;
    return TDLO_OK;
}

int tdlo_rig_self_occlusion_batch(tdlo_ctx *c, int F, const tdlo_rig_painter_frame *frames, int rows, int cols, int *visible_nodes, int *n_vis,
                                  unsigned *seen_words, unsigned *hidden_words) {
    if (!c) return TDLO_E_INVALID;
    if (F < 1 || F > 65535 || !frames || !visible_nodes || !n_vis) return fail(c, TDLO_E_INVALID, "tdlo_rig_self_occlusion_batch: 1 .. 65 535 frames, visible_nodes and n_vis");
    int Mmax = 0;
    for (int f = 0; f < F; ++f) {
        const tdlo_rig_painter_frame &q = frames[f];
        if (const char *why = rig_painter_fault(q.Y, q.M, q.cams, q.rig_to_cam, q.K, rows, cols, q.dlo_pixel_width, q.node_dist)) return fail(c, TDLO_E_INVALID, why);
        Mmax = std::max(Mmax, q.M);
    }
    PainterWords pw;
    int rc = rig_painter_enqueue(c, F, frames, rows, cols, pw);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int> vis;
    size_t iw = 0;
    for (int f = 0; f < F; ++f) {
        const tdlo_rig_painter_frame &q = frames[f];
        const size_t KW = (size_t)q.K * ((q.M + 31) / 32);
        rig_painter_verdict(pw.seen[f], pw.hidden[f], q.K, q.M, q.node_dist, q.visibility_threshold, vis);
        n_vis[f] = (int)vis.size();
        std::copy(vis.begin(), vis.end(), visible_nodes + (size_t)f * Mmax);
        if (seen_words) std::copy(pw.seen[f], pw.seen[f] + KW, seen_words + iw);
        if (hidden_words) std::copy(pw.hidden[f], pw.hidden[f] + KW, hidden_words + iw);
        iw += KW;
    }
    return TDLO_OK;
}

int tdlo_tracker_set_rig_self_occlusion(tdlo_tracker *t, const double *rig_to_cam, int K, int dlo_pixel_width) {
    if (!t) return TDLO_E_INVALID;
    if (K == 0) { t->rig_painter_K = 0; t->rig_painter_T.clear(); return TDLO_OK; }
    if (K < 1 || K > kPainterMaxCams || dlo_pixel_width < 1 || dlo_pixel_width > 255 || t->M > kPainterMaxNodes)
        return fail(t->ctx, TDLO_E_INVALID, "tdlo_tracker_set_rig_self_occlusion: 1 .. 64 cameras, dlo_pixel_width 1 .. 255, up to 1024 nodes");
    if (rig_to_cam)
        for (int k = 0; k < K; ++k) {
            bool none = true, finite = true;
            for (int q = 0; q < 12; ++q) { none = none && std::isnan(rig_to_cam[12 * k + q]); finite = finite && std::isfinite(rig_to_cam[12 * k + q]); }
            if (!none && !finite) return fail(t->ctx, TDLO_E_INVALID, "tdlo_tracker_set_rig_self_occlusion: rig_to_cam has an entry that is not finite");
        }
    t->rig_painter_K = K; t->rig_painter_width = dlo_pixel_width;
    if (rig_to_cam) t->rig_painter_T.assign(rig_to_cam, rig_to_cam + 12 * (size_t)K); else t->rig_painter_T.clear();
    return TDLO_OK;
}

// the frame of the test a tracker with the rig switch on brings to a rig call of K cameras (node_dist: the pre-pass's, read when the verdict is formed)
static tdlo_rig_painter_frame tracker_painter_frame(const tdlo_tracker *t, const tdlo_rig_camera *cams) {
    return tdlo_rig_painter_frame{t->Y.data(), t->M, cams, t->rig_painter_T.empty() ? nullptr : t->rig_painter_T.data(), t->rig_painter_K, t->rig_painter_width,
                                  t->frame_dist.data(), t->visibility_threshold};
}
// what refuses a rig call for a tracker's switches: the single switch (that test is one camera's), a rig of another camera count, what the test refuses
static const char *tracker_rig_painter_refusal(const tdlo_tracker *t, const tdlo_rig_camera *cams, int K, int rows, int cols) {
    if (t->painter_on) return "a rig frame with the self-occlusion switch on: that test is one camera's";
    if (!t->rig_painter_K) return nullptr;
    if (K != t->rig_painter_K) return "a rig frame whose camera count is not the one tdlo_tracker_set_rig_self_occlusion was given";
    static const double some_dist = 0.0;
    return rig_painter_fault(t->Y.data(), t->M, cams, t->rig_painter_T.empty() ? nullptr : t->rig_painter_T.data(), K, rows, cols, t->rig_painter_width, &some_dist);
}
// the host statement for one tracker's frame (tdlo_debug_route_count 52)
static void tracker_painter_host(tdlo_ctx *c, const tdlo_rig_painter_frame &q, int rows, int cols, std::vector<int> &vis) {
    const int W = (q.M + 31) / 32;
    std::vector<PainterCam> pc(q.K);
    for (int k = 0; k < q.K; ++k) rig_painter_camera(q.cams[k], q.rig_to_cam ? q.rig_to_cam + 12 * (size_t)k : nullptr, pc[k]);
    std::vector<unsigned> seen((size_t)q.K * W), hidden((size_t)q.K * W);
    rig_painter_host(q.Y, q.M, pc.data(), q.K, rows, cols, q.dlo_pixel_width, seen.data(), hidden.data());
    rig_painter_verdict(seen.data(), hidden.data(), q.K, q.M, q.node_dist, q.visibility_threshold, vis);
    c->pnt_route[1] += q.K;
}

// The same from a rig's images: tdlo_rig_to_cloud_visibility with the tracker's nodes into its slot, tdlo_tracker_tracking_step.  The single self-occlusion
// test is one camera's (it projects the nodes with ONE matrix): a tracker with that switch on is refused; with the rig switch on the pre-pass's visible set is
// replaced by the rig's verdict.  After a rig frame the tracker holds no camera of its own:
// tdlo_tracker_render_result wants the matrix P_k rig_to_cam_k of the camera whose image it draws over.
int tdlo_tracker_frame_from_rig(tdlo_tracker *t, const tdlo_rig_camera *cams, int K, int rows, int cols, double leaf_size, double d_vis,
                                int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                int *n_out, int *n_raw_out, tdlo_stats *stats) {
    if (!t) return TDLO_E_INVALID;
    tdlo_ctx *c = t->ctx;
    const int M = t->M;
    if (t->geodesic_coord.size() != (size_t)M) return fail(c, TDLO_E_INVALID, "the tracker has no nodes / geodesic coordinates yet (tdlo_tracker_initialize_*)");
    if (t->painter_on) return fail(c, TDLO_E_INVALID, "a rig frame with the self-occlusion switch on: that test is one camera's");
    std::vector<BatchPlanes> where;
    int rc = rig_refusal(c, t->slot, cams, K, rows, cols, leaf_size, where);
    if (rc) return rc;
    if (const char *why = tracker_rig_painter_refusal(t, cams, K, rows, cols)) return fail(c, TDLO_E_INVALID, why);
    std::vector<int> &ve = t->frame_vis_ext, &vv = t->frame_vis;
    vv.resize(M); ve.resize(M);
    int nv = 0, ne = 0, n = 0;
    t->frame_dist.resize(M);
    t->frame_Y0.clear(); t->frame_seen = false;
    rc = tdlo_rig_to_cloud_visibility(c, t->slot, cams, K, rows, cols, leaf_size, t->Y.data(), M, t->visibility_threshold, d_vis, t->geodesic_coord.data(),
                                      t->frame_dist.data(), vv.data(), &nv, ve.data(), &ne, &n, n_raw_out);
    if (!rc && n > 0 && t->rig_painter_K) {      // the rig switch: the rig's verdict on the nodes as they stand, with the pre-pass's distances; then the gap fill
        const tdlo_rig_painter_frame q = tracker_painter_frame(t, cams);
        std::vector<int> qv, qe;
        if (K >= rig_painter_min(c)) {
            PainterWords pw;
            if ((rc = rig_painter_enqueue(c, 1, &q, rows, cols, pw))) return rc;
            HIPCHK(c, hipStreamSynchronize(c->stream));
            rig_painter_verdict(pw.seen[0], pw.hidden[0], K, M, q.node_dist, q.visibility_threshold, qv);
        } else tracker_painter_host(c, q, rows, cols, qv);
        fill_visible_gaps(qv, t->geodesic_coord.data(), d_vis, qe);
        nv = (int)qv.size(); ne = (int)qe.size();
        std::copy(qv.begin(), qv.end(), vv.begin()); std::copy(qe.begin(), qe.end(), ve.begin());
    }
    if (n_out) *n_out = n;
    if (n_vis) *n_vis = nv;
    if (n_vis_ext) *n_vis_ext = ne;
    if (visible_nodes) std::copy(vv.begin(), vv.begin() + nv, visible_nodes);
    if (visible_nodes_extended) std::copy(ve.begin(), ve.begin() + ne, visible_nodes_extended);
    if (rc) return rc;
    if (n == 0) return fail(c, TDLO_E_EMPTY, "no pixel of the rig is kept: no cloud for this frame");
    if (ne == 0) return fail(c, TDLO_E_EMPTY, "no node within the visibility threshold of the cloud (the reference's callback is undefined here, trackdlo_node.cpp:351)");
    return tdlo_tracker_tracking_step(t, nullptr, 0, vv.data(), nv, ve.data(), ne, nullptr, stats);
}

// ---- F trackers in one call ----------------------------------------------------------------------
// Below this many trackers tdlo_tracker_tracking_step_batch / tdlo_tracker_frame_batch step them one by one with the single calls (which keep their short
// cuts: paired set-up, handed-over sums, the M-step launched ahead); from here on the registrations run as run_frames batches.
// Measured at production size, steady state (profiles/tracker_batch_ab.txt): two trackers 0.128 ms as batches against 0.105 ms one by one, three 0.143 against 0.158.
// TDLO_TRACKER_BATCH_MIN=n overrides (the measurement forces 2 to show both sides at every size).
constexpr int kTrackerBatchMin = 3;
static int tracker_batch_min() {
    static const int env = getenv("TDLO_TRACKER_BATCH_MIN") ? atoi(getenv("TDLO_TRACKER_BATCH_MIN")) : 0;
    return env >= 1 ? env : kTrackerBatchMin;
}

// what a batch of trackers must share (one context, distinct slots with a cloud each, node count, precision, the eleven reference parameters, nodes and
// geodesic coordinates initialised): the reason it does not, or nullptr
static const char *tracker_batch_refusal(tdlo_tracker *const *tr, int F, bool need_cloud = true) {
    if (!tr || F < 1 || !tr[0]) return "no trackers";
    const tdlo_tracker *a = tr[0];
    if (F > (int)a->ctx->slots.size()) return "more trackers than the context has slots";
    for (int i = 0; i < F; ++i) {
        const tdlo_tracker *t = tr[i];
        if (!t) return "a tracker is null";
        if (t->ctx != a->ctx) return "the trackers of a batch share one context";
        for (int j = 0; j < i; ++j) if (tr[j]->slot == t->slot) return "the trackers of a batch have distinct slots";
        if (t->M != a->M || t->precision != a->precision) return "the trackers of a batch share num_of_nodes and precision";
        if (t->visibility_threshold != a->visibility_threshold || t->beta != a->beta || t->lambda != a->lambda || t->alpha != a->alpha || t->k_vis != a->k_vis ||
            t->mu != a->mu || t->max_iter != a->max_iter || t->tol != a->tol || t->beta_pre_proc != a->beta_pre_proc || t->lambda_pre_proc != a->lambda_pre_proc ||
            t->lle_weight != a->lle_weight) return "the trackers of a batch share the reference's parameters";
        if (t->geodesic_coord.size() != (size_t)t->M || t->Y.size() != 3 * (size_t)t->M) return "a tracker has no nodes / geodesic coordinates yet (tdlo_tracker_initialize_*)";
        if (need_cloud && t->ctx->slots[t->slot].N0 <= 0) return "no cloud is resident in a tracker's slot";
    }
    return nullptr;
}

// what is wrong with the visible sets of a batch of M-node trackers, or nullptr
static const char *step_batch_sets_fault(int F, int M, const int *const *visible_nodes, const int *n_vis, const int *const *visible_nodes_extended, const int *n_vis_ext) {
    if (!visible_nodes_extended || !n_vis_ext) return "null visible_nodes_extended / n_vis_ext";
    auto nv = [&](int i) { return (visible_nodes && n_vis && visible_nodes[i]) ? n_vis[i] : 0; };
    for (int i = 0; i < F; ++i) {
        const int ne = n_vis_ext[i];
        if (!visible_nodes_extended[i] || ne <= 0 || ne > M) return "visible_nodes_extended must hold 1..M indices (empty is undefined in the reference, trackdlo_node.cpp:351)";
        for (int k = 0; k < ne; ++k) if (visible_nodes_extended[i][k] < 0 || visible_nodes_extended[i][k] >= M) return "visible_nodes_extended index out of range";
        if (nv(i) < 0) return "n_vis < 0";
        for (int k = 0; k < nv(i); ++k) if (visible_nodes[i][k] < 0 || visible_nodes[i][k] >= M) return "visible_nodes index out of range";
    }
    return nullptr;
}

int tdlo_tracker_tracking_step_batch(tdlo_tracker *const *trackers, int F, const int *const *visible_nodes, const int *n_vis,
                                     const int *const *visible_nodes_extended, const int *n_vis_ext, const double *const *H_pre,
                                     tdlo_stats *stats, int *rc_each) {
    if (!trackers || F < 1 || !trackers[0]) return TDLO_E_INVALID;
    tdlo_ctx *c = trackers[0]->ctx;
    if (const char *why = tracker_batch_refusal(trackers, F)) return fail(c, TDLO_E_INVALID, why);
    const int M = trackers[0]->M;
    if (const char *why = step_batch_sets_fault(F, M, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext)) return fail(c, TDLO_E_INVALID, why);
    auto nv = [&](int i) { return (visible_nodes && n_vis && visible_nodes[i]) ? n_vis[i] : 0; };
    std::vector<int> rcs(F, 0);
    std::vector<tdlo_stats> st(2 * (size_t)F);
    std::memset(st.data(), 0, sizeof(tdlo_stats) * st.size());
    auto finish = [&]() {
        if (stats) std::copy(st.begin(), st.end(), stats);
        if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
        for (int i = 0; i < F; ++i) if (rcs[i]) return rcs[i];
        return (int)TDLO_OK;
    };
    if (F < tracker_batch_min()) {
        for (int i = 0; i < F; ++i)
            rcs[i] = tracking_step_impl(trackers[i], nullptr, nullptr, 0, visible_nodes ? visible_nodes[i] : nullptr, nv(i), visible_nodes_extended[i], n_vis_ext[i],
                                        H_pre ? H_pre[i] : nullptr, &st[2 * (size_t)i]);
        return finish();
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (c->cloud_pending >= 0) { if (const int frc = flush_pending_cloud(c)) return frc; }
    // none of the single tracker's short cuts (PairNext, the M-step launched ahead, lle_next, the mailbox of one frame): a batch's registrations take run_frames' batch route
    c->pair.state = 0; c->pair.ahead = false; c->iter_hint = 0; c->iter_hint_next = 0;
    const tdlo_tracker *a = trackers[0];
    tdlo_params pp{};
    pp.beta = a->beta_pre_proc; pp.lambda = a->lambda_pre_proc; pp.lle_weight = a->lle_weight; pp.mu = a->mu;
    pp.max_iter = a->max_iter; pp.tol = a->tol; pp.include_lle = 1; pp.alpha = 0; pp.k_vis = 0; pp.visibility_threshold = 0.01;
    pp.precision = a->precision;
    tdlo_params mp{};
    mp.beta = a->beta; mp.lambda = a->lambda; mp.lle_weight = a->lle_weight; mp.mu = a->mu; mp.max_iter = a->max_iter;
    mp.tol = a->tol; mp.include_lle = 0; mp.alpha = a->alpha; mp.k_vis = a->k_vis; mp.visibility_threshold = a->visibility_threshold;
    mp.precision = a->precision;
    // guide nodes = visible sub-chain (:913-921), per tracker
    for (int i = 0; i < F; ++i) {
        tdlo_tracker *t = trackers[i];
        const int Mg = n_vis_ext[i];
        const int *ve = visible_nodes_extended[i];
        t->priors.clear();                                                   // :908
        t->Mg = Mg;
        t->guide_nodes.assign(3 * (size_t)Mg, 0.0);
        if (Mg != M) { for (int k = 0; k < Mg; ++k) for (int d = 0; d < 3; ++d) t->guide_nodes[d * Mg + k] = t->Y[d * M + ve[k]]; }
        else t->guide_nodes = t->Y;
    }
    // a registration's verdict per frame: the frame's own status, or -- the call failed before any frame had one -- the call's code
    auto verdicts = [&](int rc, const std::vector<int> &who, const std::vector<tdlo_stats> &sg, int which) {
        bool any = false;
        for (size_t k = 0; k < who.size(); ++k) any = any || sg[k].status != 0;
        for (size_t k = 0; k < who.size(); ++k) {
            const int i = who[k];
            rcs[i] = (rc != 0 && !any) ? rc : sg[k].status;
            st[2 * (size_t)i + which] = sg[k];
            trackers[i]->last_iters[which] = rcs[i] ? 0 : sg[k].iters;
        }
    };
    // the pre-processing registrations (:925-927), one batch per chain length n_vis_ext (steady state: one)
    std::vector<char> placed(F, 0);
    for (int i0 = 0; i0 < F; ++i0) {
        if (placed[i0]) continue;
        const int Mg = n_vis_ext[i0];
        std::vector<int> who;
        for (int i = i0; i < F; ++i) if (!placed[i] && n_vis_ext[i] == Mg) { who.push_back(i); placed[i] = 1; }
        const int Fg = (int)who.size();
        std::vector<int> sl(Fg); std::vector<double> Yg(3 * (size_t)Mg * Fg), s2(Fg); std::vector<tdlo_frame_args> ag(Fg); std::vector<tdlo_stats> sg(Fg);
        std::memset(sg.data(), 0, sizeof(tdlo_stats) * Fg);
        for (int k = 0; k < Fg; ++k) {
            const tdlo_tracker *t = trackers[who[k]];
            sl[k] = t->slot; s2[k] = t->sigma2;                              // (a copy: the pre-processing registration's sigma2 is dropped, :925)
            ag[k] = tdlo_frame_args{nullptr, 0, nullptr, 0, H_pre ? H_pre[who[k]] : nullptr};
            std::memcpy(&Yg[3 * (size_t)Mg * k], t->guide_nodes.data(), sizeof(double) * 3 * Mg);
        }
        if (Fg == 1) c->iter_hint = trackers[who[0]]->last_iters[0];
        const int rc = run_frames_each(c, Fg, sl.data(), Yg.data(), Mg, s2.data(), &pp, ag.data(), sg.data());
        c->iter_hint = 0; c->iter_hint_next = 0;
        for (int k = 0; k < Fg; ++k) std::memcpy(trackers[who[k]]->guide_nodes.data(), &Yg[3 * (size_t)Mg * k], sizeof(double) * 3 * Mg);
        verdicts(rc, who, sg, 0);
    }
    // priors per tracker (:929-995), on the host
    std::vector<int> live;
    for (int i = 0; i < F; ++i) {
        if (rcs[i]) continue;
        tdlo_tracker *t = trackers[i];
        t->vis_ext.assign(visible_nodes_extended[i], visible_nodes_extended[i] + n_vis_ext[i]);
        rcs[i] = tracker_form_priors(t, visible_nodes ? visible_nodes[i] : nullptr, nv(i));
        if (rcs[i]) t->last_iters[1] = 0; else live.push_back(i);
    }
    // the main registrations (:998) as one batch of M nodes: per-frame priors and visible_nodes_extended
    if (!live.empty()) {
        const int Fg = (int)live.size();
        std::vector<int> sl(Fg); std::vector<double> Yg(3 * (size_t)M * Fg), s2(Fg); std::vector<tdlo_frame_args> ag(Fg); std::vector<tdlo_stats> sg(Fg);
        std::memset(sg.data(), 0, sizeof(tdlo_stats) * Fg);
        for (int k = 0; k < Fg; ++k) {
            const int i = live[k];
            const tdlo_tracker *t = trackers[i];
            sl[k] = t->slot; s2[k] = t->sigma2;
            ag[k] = tdlo_frame_args{t->priors.data(), (int)(t->priors.size() / 4), visible_nodes_extended[i], n_vis_ext[i], nullptr};
            std::memcpy(&Yg[3 * (size_t)M * k], t->Y.data(), sizeof(double) * 3 * M);
        }
        if (Fg == 1) c->iter_hint = trackers[live[0]]->last_iters[1];
        const int rc = run_frames_each(c, Fg, sl.data(), Yg.data(), M, s2.data(), &mp, ag.data(), sg.data());
        for (int k = 0; k < Fg; ++k) {
            tdlo_tracker *t = trackers[live[k]];
            std::memcpy(t->Y.data(), &Yg[3 * (size_t)M * k], sizeof(double) * 3 * M);
            t->sigma2 = s2[k];
        }
        verdicts(rc, live, sg, 1);
    }
    c->iter_hint = 0; c->iter_hint_next = 0;
    c->pair.state = 0; c->pair.ahead = false; spec_abort(c);
    return finish();
}

// cell_verdict (NULL outside the occluded shared-cloud call): tracker i's visible set from the cell's words, in place of the pre-pass's.
// rigs (NULL outside the rig calls): tracker i's cameras, for the trackers whose rig switch is on -- the test under a rig replaces the pre-pass's visible set.
// From rig_painter_min jobs on k_rig_painter_batch is enqueued in front of the pre-pass and its words are read after that call's wait: no wait is added
static int tracker_frame_batch_impl(tdlo_tracker *const *trackers, int F, double d_vis, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                                    tdlo_stats *stats, int *rc_each, const tdlo_rig_camera *const *rigs, int rows, int cols, const double *pre_min_d2 = nullptr,
                                    const std::function<void(int, const tdlo_tracker *, std::vector<int> &)> *cell_verdict = nullptr) {
    if (!trackers || F < 1 || !trackers[0]) return TDLO_E_INVALID;
    tdlo_ctx *c = trackers[0]->ctx;
    if (const char *why = tracker_batch_refusal(trackers, F)) return fail(c, TDLO_E_INVALID, why);
    const int M = trackers[0]->M;
    std::vector<tdlo_rig_painter_frame> pf;      // the frames of the test, and whose they are
    std::vector<int> pf_of(F, -1);
    PainterWords pw;
    bool painter_kernel = false;
    if (rigs) {
        int jobs = 0;
        for (int i = 0; i < F; ++i)
            if (trackers[i]->rig_painter_K && rigs[i]) {
                trackers[i]->frame_dist.resize(M);
                pf_of[i] = (int)pf.size();
                pf.push_back(tracker_painter_frame(trackers[i], rigs[i]));
                jobs += trackers[i]->rig_painter_K;
            }
        if (!pf.empty() && jobs >= rig_painter_min(c)) {
            const int prc = rig_painter_enqueue(c, (int)pf.size(), pf.data(), rows, cols, pw);
            if (prc) return prc;
            painter_kernel = true;
        }
    }
    std::vector<int> sl(F), nv(F, 0), ne(F, 0), vis((size_t)F * M), ext((size_t)F * M);
    std::vector<double> Yall(3 * (size_t)M * F), coord((size_t)M * F), dist((size_t)M * F);
    for (int i = 0; i < F; ++i) {
        const tdlo_tracker *t = trackers[i];
        sl[i] = t->slot;
        std::memcpy(&Yall[3 * (size_t)M * i], t->Y.data(), sizeof(double) * 3 * M);
        std::memcpy(&coord[(size_t)M * i], t->geodesic_coord.data(), sizeof(double) * M);
    }
    int rc = 0;
    if (pre_min_d2)      // (the squared minima came with the clouds: the pre-pass rode in k_assign_scatter)
        for (int i = 0; i < F; ++i)
            vis_threshold_and_fill(pre_min_d2 + (size_t)M * i, M, trackers[0]->visibility_threshold, d_vis, &coord[(size_t)M * i], &dist[(size_t)M * i], &vis[(size_t)M * i],
                                   &nv[i], &ext[(size_t)M * i], &ne[i]);
    else
        rc = tdlo_visibility_prepass_batch(c, F, sl.data(), Yall.data(), M, trackers[0]->visibility_threshold, d_vis, coord.data(), dist.data(), vis.data(), nv.data(),
                                           ext.data(), ne.data());
    if (rc) {
        if (painter_kernel) (void)hipStreamSynchronize(c->stream);      // (the words are not read; nothing of this call stays in flight)
        return rc;
    }
    std::vector<tdlo_tracker *> sub;
    std::vector<const int *> pv, pe;
    std::vector<int> snv, sne, who;
    for (int i = 0; i < F; ++i) {
        tdlo_tracker *t = trackers[i];
        int *v = &vis[(size_t)M * i], *e = &ext[(size_t)M * i];
        t->frame_dist.assign(&dist[(size_t)M * i], &dist[(size_t)M * i] + M);
        if (t->painter_on) t->frame_Y0 = t->Y; else t->frame_Y0.clear();
        if (t->painter_on) {      // the self-occlusion switch, as in tracker_frame_impl
            std::vector<int> qv, qe;
            self_occlusion_visible(t->Y.data(), M, t->painter_proj, t->painter_width, t->frame_dist.data(), t->visibility_threshold, qv);
            fill_visible_gaps(qv, t->geodesic_coord.data(), d_vis, qe);
            nv[i] = (int)qv.size(); ne[i] = (int)qe.size();
            std::copy(qv.begin(), qv.end(), v); std::copy(qe.begin(), qe.end(), e);
        }
        if (pf_of[i] >= 0) {      // the rig switch: the rig's verdict with the pre-pass's distances, then the gap fill
            tdlo_rig_painter_frame &q = pf[pf_of[i]];
            q.node_dist = t->frame_dist.data();
            std::vector<int> qv, qe;
            if (painter_kernel) rig_painter_verdict(pw.seen[pf_of[i]], pw.hidden[pf_of[i]], q.K, M, q.node_dist, q.visibility_threshold, qv);
            else tracker_painter_host(c, q, rows, cols, qv);
            fill_visible_gaps(qv, t->geodesic_coord.data(), d_vis, qe);
            nv[i] = (int)qv.size(); ne[i] = (int)qe.size();
            std::copy(qv.begin(), qv.end(), v); std::copy(qe.begin(), qe.end(), e);
        }
        if (cell_verdict) {      // the cell's verdict on this rope (tdlo_tracker_frames_from_shared_cloud_occluded_batch) with the pre-pass's distances, then the gap fill
            std::vector<int> qv, qe;
            (*cell_verdict)(i, t, qv);
            fill_visible_gaps(qv, t->geodesic_coord.data(), d_vis, qe);
            nv[i] = (int)qv.size(); ne[i] = (int)qe.size();
            std::copy(qv.begin(), qv.end(), v); std::copy(qe.begin(), qe.end(), e);
        }
        t->frame_vis.assign(v, v + M); t->frame_vis_ext.assign(e, e + M);
        if (ne[i] > 0) { sub.push_back(t); pv.push_back(v); pe.push_back(e); snv.push_back(nv[i]); sne.push_back(ne[i]); who.push_back(i); }
    }
    if (visible_nodes) std::copy(vis.begin(), vis.end(), visible_nodes);
    if (visible_nodes_extended) std::copy(ext.begin(), ext.end(), visible_nodes_extended);
    if (n_vis) std::copy(nv.begin(), nv.end(), n_vis);
    if (n_vis_ext) std::copy(ne.begin(), ne.end(), n_vis_ext);
    std::vector<int> rcs(F, 0), src(sub.size(), 0);
    std::vector<tdlo_stats> st(2 * (size_t)F), sst(2 * sub.size() + 2);
    std::memset(st.data(), 0, sizeof(tdlo_stats) * st.size());
    std::memset(sst.data(), 0, sizeof(tdlo_stats) * sst.size());
    // (the reference's callback indexes visible_nodes[size() - 1] without a test, trackdlo_node.cpp:351-361: a frame without a visible node is an error here)
    for (int i = 0; i < F; ++i) if (ne[i] == 0) rcs[i] = TDLO_E_EMPTY;
    if (!sub.empty()) {
        const int brc = tdlo_tracker_tracking_step_batch(sub.data(), (int)sub.size(), pv.data(), snv.data(), pe.data(), sne.data(), nullptr, sst.data(), src.data());
        for (size_t k = 0; k < sub.size(); ++k) {
            rcs[who[k]] = src[k] ? src[k] : 0;
            st[2 * (size_t)who[k]] = sst[2 * k]; st[2 * (size_t)who[k] + 1] = sst[2 * k + 1];
        }
        bool any = false;
        for (int r : src) any = any || r != 0;
        if (brc && !any) return brc;      // (refused as a whole: nothing was stepped)
    }
    if (stats) std::copy(st.begin(), st.end(), stats);
    if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
    for (int i = 0; i < F; ++i)
        if (rcs[i]) return rcs[i] == TDLO_E_EMPTY && ne[i] == 0
                               ? fail(c, TDLO_E_EMPTY, "no node within the visibility threshold of the cloud (the reference's callback is undefined here, trackdlo_node.cpp:351)") : rcs[i];
    return TDLO_OK;
}

int tdlo_tracker_frame_batch(tdlo_tracker *const *trackers, int F, double d_vis, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext,
                             tdlo_stats *stats, int *rc_each) {
    return tracker_frame_batch_impl(trackers, F, d_vis, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext, stats, rc_each, nullptr, 0, 0);
}

// The frames of F trackers from their images: tdlo_depth_to_cloud_batch into the trackers' slots, then tdlo_tracker_frame_batch on the trackers that got a cloud
// clouds: the entrance's cloud batch call over the frames (frames, n, n_raw, rc_each); cam: the camera of image k, read once the cloud call has accepted the images
static int tracker_frames_batch_common(tdlo_tracker *const *trackers, int F, const int *image_of, const tdlo_colour_params *const *colour_params,
                                       const std::function<int(tdlo_ctx *, const tdlo_batch_frame *, int *, int *, int *)> &clouds,
                                       const std::function<void(int, double *)> &cam, double d_vis,
                                       int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext, int *n_out, int *n_raw_out, tdlo_stats *stats, int *rc_each) {
    if (!trackers || F < 1 || !trackers[0]) return TDLO_E_INVALID;
    tdlo_ctx *c = trackers[0]->ctx;
    if (const char *why = tracker_batch_refusal(trackers, F, false)) return fail(c, TDLO_E_INVALID, why);
    if (!image_of) return fail(c, TDLO_E_INVALID, "null image_of");
    const int M = trackers[0]->M;
    std::vector<tdlo_batch_frame> fr(F);
    for (int i = 0; i < F; ++i) fr[i] = tdlo_batch_frame{trackers[i]->slot, image_of[i], colour_params ? colour_params[i] : nullptr};
    std::vector<int> n(F, 0), nraw(F, 0), rcs(F, 0);
    int rc = clouds(c, fr.data(), n.data(), nraw.data(), rcs.data());
    if (n_out) std::copy(n.begin(), n.end(), n_out);
    if (n_raw_out) std::copy(nraw.begin(), nraw.end(), n_raw_out);
    bool any = false;
    for (int r : rcs) any = any || r != 0;
    if (rc && !any) return rc;                     // (refused as a whole: nothing was touched)
    std::vector<tdlo_tracker *> sub;
    std::vector<int> who;
    for (int i = 0; i < F; ++i) {
        if (!rcs[i] && n[i] == 0) rcs[i] = TDLO_E_EMPTY;      // the frame selects no pixel: no cloud, the tracker is left as it is
        if (!rcs[i]) {
            tdlo_tracker *t = trackers[i];
            cam(image_of[i], t->frame_cam);
            t->frame_seen = true;
            sub.push_back(t); who.push_back(i);
        }
    }
    std::vector<tdlo_stats> st(2 * (size_t)F);
    std::memset(st.data(), 0, sizeof(tdlo_stats) * st.size());
    std::vector<int> nv(F, 0), ne(F, 0), vis((size_t)F * M, 0), ext((size_t)F * M, 0);
    if (!sub.empty()) {
        const int Fs = (int)sub.size();
        std::vector<int> snv(Fs, 0), sne(Fs, 0), svis((size_t)Fs * M, 0), sext((size_t)Fs * M, 0), src(Fs, 0);
        std::vector<tdlo_stats> sst(2 * (size_t)Fs);
        std::memset(sst.data(), 0, sizeof(tdlo_stats) * sst.size());
        const int brc = tdlo_tracker_frame_batch(sub.data(), Fs, d_vis, svis.data(), snv.data(), sext.data(), sne.data(), sst.data(), src.data());
        bool sany = false;
        for (int r : src) sany = sany || r != 0;
        for (int k = 0; k < Fs; ++k) {
            const int i = who[k];
            rcs[i] = (brc && !sany) ? brc : src[k];
            nv[i] = snv[k]; ne[i] = sne[k];
            std::copy(&svis[(size_t)M * k], &svis[(size_t)M * k] + M, &vis[(size_t)M * i]);
            std::copy(&sext[(size_t)M * k], &sext[(size_t)M * k] + M, &ext[(size_t)M * i]);
            st[2 * (size_t)i] = sst[2 * (size_t)k]; st[2 * (size_t)i + 1] = sst[2 * (size_t)k + 1];
        }
    }
    if (visible_nodes) std::copy(vis.begin(), vis.end(), visible_nodes);
    if (visible_nodes_extended) std::copy(ext.begin(), ext.end(), visible_nodes_extended);
    if (n_vis) std::copy(nv.begin(), nv.end(), n_vis);
    if (n_vis_ext) std::copy(ne.begin(), ne.end(), n_vis_ext);
    if (stats) std::copy(st.begin(), st.end(), stats);
    if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
    for (int i = 0; i < F; ++i)
        if (rcs[i]) return (rcs[i] == TDLO_E_EMPTY && n[i] == 0) ? fail(c, TDLO_E_EMPTY, "the mask selects no pixel: no cloud for this frame") : rcs[i];
    return TDLO_OK;
}

int tdlo_tracker_frames_batch(tdlo_tracker *const *trackers, int F, const tdlo_batch_image *images, int K, int rows, int cols, const int *image_of,
                              const tdlo_colour_params *const *colour_params, double leaf_size, double d_vis,
                              int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext, int *n_out, int *n_raw_out, tdlo_stats *stats, int *rc_each) {
    return tracker_frames_batch_common(
        trackers, F, image_of, colour_params,
        [&](tdlo_ctx *c, const tdlo_batch_frame *fr, int *n, int *nraw, int *rcs) { return tdlo_depth_to_cloud_batch(c, images, K, rows, cols, fr, F, leaf_size, n, nraw, rcs); },
        [&](int k, double *cam) { cam[0] = images[k].fx; cam[1] = images[k].fy; cam[2] = images[k].cx; cam[3] = images[k].cy; }, d_vis, visible_nodes, n_vis,
        visible_nodes_extended, n_vis_ext, n_out, n_raw_out, stats, rc_each);
}

// The same from image views: tdlo_frame_views_to_cloud_batch (under the tracker entrance's crossover) into the trackers' slots, then tdlo_tracker_frame_batch
int tdlo_tracker_frame_views_batch(tdlo_tracker *const *trackers, int F, const tdlo_view_image *images, int K, int rows, int cols, const int *image_of,
                                   const tdlo_colour_params *const *colour_params, double leaf_size, double d_vis,
                                   int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext, int *n_out, int *n_raw_out, tdlo_stats *stats, int *rc_each) {
    return tracker_frames_batch_common(
        trackers, F, image_of, colour_params,
        [&](tdlo_ctx *c, const tdlo_batch_frame *fr, int *n, int *nraw, int *rcs) { return frame_views_batch_impl(c, images, K, rows, cols, fr, F, leaf_size, n, nraw, rcs, true); },
        [&](int k, double *cam) { cam[0] = images[k].fx; cam[1] = images[k].fy; cam[2] = images[k].cx; cam[3] = images[k].cy; }, d_vis, visible_nodes, n_vis,
        visible_nodes_extended, n_vis_ext, n_out, n_raw_out, stats, rc_each);
}

// tracking_step of F trackers on clouds where they lie: tdlo_set_cloud_view_batch into the trackers' slots, enqueued (the registrations wait for the stream
// before the call returns), then tdlo_tracker_tracking_step_batch
int tdlo_tracker_tracking_step_view_batch(tdlo_tracker *const *trackers, int F, const tdlo_cloud_view *const *views, const int *N,
                                          const int *const *visible_nodes, const int *n_vis, const int *const *visible_nodes_extended, const int *n_vis_ext,
                                          const double *const *H_pre, tdlo_stats *stats, int *rc_each) {
    if (!trackers || F < 1 || !trackers[0]) return TDLO_E_INVALID;
    tdlo_ctx *c = trackers[0]->ctx;
    if (const char *why = tracker_batch_refusal(trackers, F, false)) return fail(c, TDLO_E_INVALID, why);
    if (const char *why = step_batch_sets_fault(F, trackers[0]->M, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext)) return fail(c, TDLO_E_INVALID, why);
    std::vector<int> slots(F), rcs(F, 0);
    for (int i = 0; i < F; ++i) slots[i] = trackers[i]->slot;
    int rc = view_import_batch_impl(c, slots.data(), views, N, F, rcs.data(), false, true);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);          // (whatever was enqueued has left the pinned block before the caller hears of the failure)
        if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
        return rc;
    }
    rc = tdlo_tracker_tracking_step_batch(trackers, F, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext, H_pre, stats, rc_each);
    if (rc) (void)hipStreamSynchronize(c->stream);
    return rc;
}

// The frames of F trackers from clouds where they lie: tdlo_cloud_view_voxel_grid_batch into the trackers' slots, then tdlo_tracker_frame_batch on the trackers
// that got a cloud (tdlo_tracker_frames_batch with views where it has images)
int tdlo_tracker_frames_from_cloud_view_batch(tdlo_tracker *const *trackers, int F, const tdlo_view_frame *frames, double leaf_size, double d_vis,
                                              int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext, int *n_out, int *n_raw_out,
                                              tdlo_stats *stats, int *rc_each) {
    if (!trackers || F < 1 || !trackers[0]) return TDLO_E_INVALID;
    tdlo_ctx *c = trackers[0]->ctx;
    if (const char *why = tracker_batch_refusal(trackers, F, false)) return fail(c, TDLO_E_INVALID, why);
    if (!frames) return fail(c, TDLO_E_INVALID, "null frames");
    const int M = trackers[0]->M;
    std::vector<tdlo_view_frame> fr(frames, frames + F);
    for (int i = 0; i < F; ++i) fr[i].slot = trackers[i]->slot;
    std::vector<int> n(F, 0), nraw(F, 0), rcs(F, 0);
    int rc = view_voxel_batch_frames(c, fr.data(), F, leaf_size, n.data(), nraw.data(), rcs.data(), true);
    if (n_out) std::copy(n.begin(), n.end(), n_out);
    if (n_raw_out) std::copy(nraw.begin(), nraw.end(), n_raw_out);
    bool any = false;
    for (int r : rcs) any = any || r != 0;
    if (rc && !any) return rc;                     // (refused as a whole: nothing was touched)
    std::vector<tdlo_tracker *> sub;
    std::vector<int> who;
    for (int i = 0; i < F; ++i) {
        if (!rcs[i] && n[i] == 0) rcs[i] = TDLO_E_EMPTY;      // the view keeps no point: no cloud, the tracker is left as it is
        if (!rcs[i]) { sub.push_back(trackers[i]); who.push_back(i); }
    }
    std::vector<tdlo_stats> st(2 * (size_t)F);
    std::memset(st.data(), 0, sizeof(tdlo_stats) * st.size());
    std::vector<int> nv(F, 0), ne(F, 0), vis((size_t)F * M, 0), ext((size_t)F * M, 0);
    if (!sub.empty()) {
        const int Fs = (int)sub.size();
        std::vector<int> snv(Fs, 0), sne(Fs, 0), svis((size_t)Fs * M, 0), sext((size_t)Fs * M, 0), src(Fs, 0);
        std::vector<tdlo_stats> sst(2 * (size_t)Fs);
        std::memset(sst.data(), 0, sizeof(tdlo_stats) * sst.size());
        const int brc = tdlo_tracker_frame_batch(sub.data(), Fs, d_vis, svis.data(), snv.data(), sext.data(), sne.data(), sst.data(), src.data());
        bool sany = false;
        for (int r : src) sany = sany || r != 0;
        for (int k = 0; k < Fs; ++k) {
            const int i = who[k];
            rcs[i] = (brc && !sany) ? brc : src[k];
            nv[i] = snv[k]; ne[i] = sne[k];
            std::copy(&svis[(size_t)M * k], &svis[(size_t)M * k] + M, &vis[(size_t)M * i]);
            std::copy(&sext[(size_t)M * k], &sext[(size_t)M * k] + M, &ext[(size_t)M * i]);
            st[2 * (size_t)i] = sst[2 * (size_t)k]; st[2 * (size_t)i + 1] = sst[2 * (size_t)k + 1];
        }
    }
    if (visible_nodes) std::copy(vis.begin(), vis.end(), visible_nodes);
    if (visible_nodes_extended) std::copy(ext.begin(), ext.end(), visible_nodes_extended);
    if (n_vis) std::copy(nv.begin(), nv.end(), n_vis);
    if (n_vis_ext) std::copy(ne.begin(), ne.end(), n_vis_ext);
    if (stats) std::copy(st.begin(), st.end(), stats);
    if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
    for (int i = 0; i < F; ++i)
        if (rcs[i]) return (rcs[i] == TDLO_E_EMPTY && n[i] == 0) ? fail(c, TDLO_E_EMPTY, "the view keeps no point: no cloud for this frame") : rcs[i];
    return TDLO_OK;
}

// The frames of F trackers from F rigs: tdlo_rig_to_cloud_batch into the trackers' slots (frames[i].slot is not read), then tdlo_tracker_frame_batch on the
// trackers that got a cloud.  The self-occlusion test is one camera's: a tracker with the switch on refuses the call, as tdlo_tracker_frame_from_rig refuses it
int tdlo_tracker_frames_from_rig_batch(tdlo_tracker *const *trackers, int F, const tdlo_rig_frame *frames, int rows, int cols, double leaf_size, double d_vis,
                                       int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext, int *n_out, int *n_raw_out,
                                       tdlo_stats *stats, int *rc_each) {
    if (!trackers || F < 1 || !trackers[0]) return TDLO_E_INVALID;
    tdlo_ctx *c = trackers[0]->ctx;
    if (const char *why = tracker_batch_refusal(trackers, F, false)) return fail(c, TDLO_E_INVALID, why);
    if (!frames) return fail(c, TDLO_E_INVALID, "null frames");
    for (int i = 0; i < F; ++i)
        if (trackers[i]->painter_on) return fail(c, TDLO_E_INVALID, "a rig frame with the self-occlusion switch on: that test is one camera's");
    bool any_painter = false;
    for (int i = 0; i < F; ++i) {
        if (!trackers[i]->rig_painter_K) continue;
        any_painter = true;
        if (!frames[i].cams) return fail(c, TDLO_E_INVALID, "rig: no cameras");
        if (const char *why = tracker_rig_painter_refusal(trackers[i], frames[i].cams, frames[i].K, rows, cols)) return fail(c, TDLO_E_INVALID, why);
    }
    const int M = trackers[0]->M;
    std::vector<tdlo_rig_frame> fr(frames, frames + F);
    for (int i = 0; i < F; ++i) fr[i].slot = trackers[i]->slot;
    std::vector<int> n(F, 0), nraw(F, 0), rcs(F, 0);
    int rc = rig_batch_impl(c, fr.data(), F, rows, cols, leaf_size, n.data(), nraw.data(), rcs.data(), true);
    if (n_out) std::copy(n.begin(), n.end(), n_out);
    if (n_raw_out) std::copy(nraw.begin(), nraw.end(), n_raw_out);
    bool any = false;
    for (int r : rcs) any = any || r != 0;
    if (rc && !any) return rc;                     // (refused as a whole: nothing was touched)
    std::vector<tdlo_tracker *> sub;
    std::vector<int> who;
    for (int i = 0; i < F; ++i) {
        if (!rcs[i] && n[i] == 0) rcs[i] = TDLO_E_EMPTY;      // the rig keeps no pixel: no cloud, the tracker is left as it is
        if (!rcs[i]) { trackers[i]->frame_seen = false; sub.push_back(trackers[i]); who.push_back(i); }      // (after a rig frame the tracker holds no camera of its own)
    }
    std::vector<const tdlo_rig_camera *> rigs;      // the rig switch: the cameras of the trackers that go on
    if (any_painter) for (int i : who) rigs.push_back(frames[i].cams);
    std::vector<tdlo_stats> st(2 * (size_t)F);
    std::memset(st.data(), 0, sizeof(tdlo_stats) * st.size());
    std::vector<int> nv(F, 0), ne(F, 0), vis((size_t)F * M, 0), ext((size_t)F * M, 0);
    if (!sub.empty()) {
        const int Fs = (int)sub.size();
        std::vector<int> snv(Fs, 0), sne(Fs, 0), svis((size_t)Fs * M, 0), sext((size_t)Fs * M, 0), src(Fs, 0);
        std::vector<tdlo_stats> sst(2 * (size_t)Fs);
        std::memset(sst.data(), 0, sizeof(tdlo_stats) * sst.size());
        const int brc = tracker_frame_batch_impl(sub.data(), Fs, d_vis, svis.data(), snv.data(), sext.data(), sne.data(), sst.data(), src.data(),
                                                 any_painter ? rigs.data() : nullptr, rows, cols);
        bool sany = false;
        for (int r : src) sany = sany || r != 0;
        for (int k = 0; k < Fs; ++k) {
            const int i = who[k];
            rcs[i] = (brc && !sany) ? brc : src[k];
            nv[i] = snv[k]; ne[i] = sne[k];
            std::copy(&svis[(size_t)M * k], &svis[(size_t)M * k] + M, &vis[(size_t)M * i]);
            std::copy(&sext[(size_t)M * k], &sext[(size_t)M * k] + M, &ext[(size_t)M * i]);
            st[2 * (size_t)i] = sst[2 * (size_t)k]; st[2 * (size_t)i + 1] = sst[2 * (size_t)k + 1];
        }
    }
    if (visible_nodes) std::copy(vis.begin(), vis.end(), visible_nodes);
    if (visible_nodes_extended) std::copy(ext.begin(), ext.end(), visible_nodes_extended);
    if (n_vis) std::copy(nv.begin(), nv.end(), n_vis);
    if (n_vis_ext) std::copy(ne.begin(), ne.end(), n_vis_ext);
    if (stats) std::copy(st.begin(), st.end(), stats);
    if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
    for (int i = 0; i < F; ++i)
        if (rcs[i]) return (rcs[i] == TDLO_E_EMPTY && n[i] == 0) ? fail(c, TDLO_E_EMPTY, "no pixel of the rig is kept: no cloud for this frame") : rcs[i];
    return TDLO_OK;
}

// ---- raw depth for many cameras in one call (include/trackdlo_hip.h: tdlo_align_depth_batch and the aligning rig calls; tdlo_align_batch.hip the kernels,
// tdlo_align_batch_plan.h the arena) ---------------------------------------------------------------------------------------------------------------------
// From this many jobs on a call takes the batch launches; below it it loops launch_align into the arena's planes (the same bits, no host wait either).  The rule,
// set beforehand (scripts/gpu_align_batch.py -> profiles/align_batch_ab.txt): the smallest J from which every batch value lies below every looped value on all
// four lines (640 x 480 -> 640 x 480 and 848 x 480 -> 1280 x 720, device and pageable host depth), 1025 where no J up to 32 qualifies.  NOT MEASURED YET: 1025,
// the call loops by default; TDLO_ALIGN_BATCH_MIN=n (read when the context is made) overrides.
constexpr int kAlignBatchMin = 1025;
static int align_batch_min(const tdlo_ctx *c) { return c->align_batch_min ? c->align_batch_min : kAlignBatchMin; }
constexpr size_t kAlnbPinCounts = 32 * (size_t)kAlignBatchMaxJobs;                                      // the pack kernel's 4 x 1024 result words
constexpr size_t kAlnbPinHead = kAlnbPinCounts + 32 * (size_t)kAlignBatchMaxJobs + sizeof(AlignBatchRec) * (size_t)kAlignBatchMaxJobs;

int tdlo_debug_align_batch_plan(const int *rows_c, const int *cols_c, int J, long long budget, long long *scratch_off, long long *plane_off,
                                long long *counts_off, long long *table_off, long long *scratch_bytes, long long *total) {
    return align_batch_plan(rows_c, cols_c, J, budget > 0 ? budget : kAlignBatchBudget, scratch_off, plane_off, counts_off, table_off, scratch_bytes, total) ? TDLO_E_INVALID : TDLO_OK;
}

int tdlo_debug_align_batch_arena(tdlo_ctx *c, const void **base, long long *bytes) {
    if (!c || !base || !bytes) return TDLO_E_INVALID;
    *base = c->alnb_dev; *bytes = (long long)c->alnb_cap;
    return TDLO_OK;
}

int tdlo_debug_align_distinct_jobs(const tdlo_align_job *entries, int n, int *job_of) {
    if (!entries || !job_of || n < 1) return TDLO_E_INVALID;
    std::vector<tdlo_image_view> v(n);
    std::vector<tdlo_align_params> p(n);
    for (int e = 0; e < n; ++e) { v[e] = entries[e].depth; p[e] = entries[e].p; }
    return align_distinct_jobs(v.data(), p.data(), n, job_of);
}

// A checked batch as the enqueue takes it: where every view lies, the plan, which jobs share an uploaded host view
struct AlignBatchWork {
    int J = 0;
    std::vector<char> dev;                                  // job j's depth view lies in device memory
    std::vector<long long> scratch_off, plane_off, counts_off;
    long long table_off = 0, scratch_bytes = 0, total = 0;
    std::vector<int> up_of;                                 // a host view's upload (-1: a device view); jobs that name one view share it
    std::vector<size_t> up_at;                              // per upload: bytes from the start of the packed block
    size_t up_bytes = 0;
    int most_Pd = 0, most_Pc = 0;
};

static bool alnb_overlaps(const tdlo_ctx *c, const char *a, const char *b) {      // [a, b) against the arena and the upload block
    return (c->alnb_dev && a < c->alnb_dev + c->alnb_cap && b > c->alnb_dev) || (c->alnb_up && a < c->alnb_up + c->alnb_up_cap && b > c->alnb_up);
}

// Everything that refuses a batch as a whole; nothing of the context is touched.  aligned_out may be null; out_dev (may be null): which outputs are device memory
static int align_batch_refusal(tdlo_ctx *c, const tdlo_align_job *jobs, int J, unsigned short *const *aligned_out, AlignBatchWork &w, std::vector<char> *out_dev) {
    if (!jobs || J < 1 || J > kAlignBatchMaxJobs) return fail(c, TDLO_E_INVALID, "align batch: 1 .. 1024 jobs");
    for (int j = 0; j < J; ++j)
        if (int rc = align_refusal(c, &jobs[j].depth, &jobs[j].p)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    w.J = J;
    w.dev.assign(J, 0); w.up_of.assign(J, -1); w.up_at.clear(); w.up_bytes = 0; w.most_Pd = w.most_Pc = 0;
    if (out_dev) out_dev->assign(J, 0);
    std::vector<int> rows(J), cols(J);
    for (int j = 0; j < J; ++j) {
        const tdlo_align_params &p = jobs[j].p;
        bool dev = false;
        if (int rc = image_view_where(c, &jobs[j].depth, p.rows_d, p.cols_d, &dev)) return rc;
        w.dev[j] = dev;
        if (dev) {
            long long lo, hi;
            image_view_span(&jobs[j].depth, p.rows_d, p.cols_d, &lo, &hi);
            if (alnb_overlaps(c, (const char *)jobs[j].depth.data + lo, (const char *)jobs[j].depth.data + hi))
                return fail(c, TDLO_E_INVALID, "align batch: a device view overlaps the arena");
        }
        if (aligned_out && aligned_out[j]) {
            bool od = false;
            if (int rc = pointer_location(c, aligned_out[j], TDLO_MEM_AUTO, "align batch: aligned_out", &od)) return rc;
            if (od && alnb_overlaps(c, (const char *)aligned_out[j], (const char *)aligned_out[j] + 2 * (size_t)p.rows_c * p.cols_c))
                return fail(c, TDLO_E_INVALID, "align batch: a device aligned_out overlaps the arena");
            if (out_dev) (*out_dev)[j] = od;
        }
        rows[j] = p.rows_c; cols[j] = p.cols_c;
        w.most_Pd = std::max(w.most_Pd, p.rows_d * p.cols_d); w.most_Pc = std::max(w.most_Pc, p.rows_c * p.cols_c);
    }
    w.scratch_off.assign(J, 0); w.plane_off.assign(J, 0); w.counts_off.assign(J, 0);
    if (align_batch_plan(rows.data(), cols.data(), J, kAlignBatchBudget, w.scratch_off.data(), w.plane_off.data(), w.counts_off.data(), &w.table_off, &w.scratch_bytes, &w.total))
        return fail(c, TDLO_E_INVALID, "align batch: the arena of these jobs would pass 1 GiB");
    // the packed block: every depth image the host has to hold -- on the device route the host views (one named by several jobs once), on the host route all
    for (int j = 0; j < J; ++j) {
        if (w.dev[j] && !c->align_host) continue;
        const tdlo_image_view &v = jobs[j].depth;
        for (int i = 0; i < j && w.up_of[j] < 0; ++i) {
            const tdlo_image_view &u = jobs[i].depth;
            if (w.up_of[i] >= 0 && u.data == v.data && u.format == v.format && u.row_stride == v.row_stride && u.location == v.location && u.ready_stream == v.ready_stream &&
                jobs[i].p.rows_d == jobs[j].p.rows_d && jobs[i].p.cols_d == jobs[j].p.cols_d) w.up_of[j] = w.up_of[i];
        }
        if (w.up_of[j] >= 0) continue;
        w.up_of[j] = (int)w.up_at.size();
        w.up_at.push_back(w.up_bytes);
        w.up_bytes += aln_round(2 * (size_t)jobs[j].p.rows_d * jobs[j].p.cols_d);
    }
    return TDLO_OK;
}

// The planes of a checked batch, enqueued on the context's stream WITHOUT a host wait on the device routes: planes[j] (J entries) are the arena's.  The counts
// are the caller's after the stream's next wait (align_batch_counts_fetch)
static int align_batch_enqueue(tdlo_ctx *c, const tdlo_align_job *jobs, AlignBatchWork &w, const unsigned short **planes) {
    const int J = w.J;
    hipStream_t st = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->alnb_up_pending) { HIPCHK(c, hipEventSynchronize(c->alnb_ev_up)); c->alnb_up_pending = false; }      // the pinned block is about to be rewritten
    // ---- room: the arena (a new one is filled where its scratch region lies), the upload block, the pinned block
    const size_t plane_bytes = (size_t)(w.counts_off[0] - w.plane_off[0]);
    const size_t pin_need = kAlnbPinHead + w.up_bytes + (c->align_host ? plane_bytes : 0);
    if ((size_t)w.total > c->alnb_cap || w.up_bytes > c->alnb_up_cap || pin_need > c->alnb_pin_cap) HIPCHK(c, drain_for_realloc(c));
    if ((size_t)w.total > c->alnb_cap) {
        if (c->alnb_dev) hipFree(c->alnb_dev);
        c->alnb_dev = nullptr; c->alnb_cap = 0; c->alnb_armed = 0;
        HIPCHK(c, hipMalloc((void **)&c->alnb_dev, (size_t)w.total));
        c->alnb_cap = (size_t)w.total;
    }
    if (w.up_bytes > c->alnb_up_cap) {
        if (c->alnb_up) hipFree(c->alnb_up);
        c->alnb_up = nullptr; c->alnb_up_cap = 0;
        HIPCHK(c, hipMalloc((void **)&c->alnb_up, w.up_bytes));
        c->alnb_up_cap = w.up_bytes;
    }
    if (pin_need > c->alnb_pin_cap) {
        if (c->alnb_pin) hipHostFree(c->alnb_pin);
        c->alnb_pin = nullptr; c->alnb_pin_cap = 0;
        HIPCHK(c, hipHostMalloc((void **)&c->alnb_pin, pin_need, hipHostMallocDefault));
        c->alnb_pin_cap = pin_need;
        std::memset(c->alnb_pin, 0, kAlnbPinCounts);
    }
    if (!c->alnb_ev_up) HIPCHK(c, hipEventCreateWithFlags(&c->alnb_ev_up, hipEventDisableTiming));
    char *arena = c->alnb_dev, *pin_up = c->alnb_pin + kAlnbPinHead;
    for (int j = 0; j < J; ++j) planes[j] = (const unsigned short *)(arena + w.plane_off[j]);
    // ---- one event per distinct ready_stream of the device views
    {
        std::vector<void *> seen;
        for (int j = 0; j < J; ++j) {
            void *rs = jobs[j].depth.ready_stream;
            if (!w.dev[j] || !rs || std::find(seen.begin(), seen.end(), rs) != seen.end()) continue;
            if (seen.size() == c->alnb_ev.size()) {
                hipEvent_t e = nullptr;
                HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
                c->alnb_ev.push_back(e);
            }
            HIPCHK(c, hipEventRecord(c->alnb_ev[seen.size()], (hipStream_t)rs));
            HIPCHK(c, hipStreamWaitEvent(st, c->alnb_ev[seen.size()], 0));
            seen.push_back(rs);
        }
    }
    if (c->align_host) {
        // the comparator: every plane from the host statement, uploaded in one copy.  Device views come down as their packed canonical depth (k_image_import)
        bool any_dev = false;
        std::vector<char> done(w.up_at.size(), 0);
        for (int j = 0; j < J; ++j) {
            const int u = w.up_of[j];
            if (done[u]) continue;
            done[u] = 1;
            const tdlo_align_params &p = jobs[j].p;
            const size_t Pd = (size_t)p.rows_d * p.cols_d;
            if (!w.dev[j]) { image_pack_host(&jobs[j].depth, p.rows_d, p.cols_d, pin_up + w.up_at[u]); continue; }
            ImageJob ij{};
            ij.P = (int)Pd; ij.cols = p.cols_d;
            ij.src[kRoleDepth] = ImageSrc{(const unsigned char *)jobs[j].depth.data, jobs[j].depth.row_stride, jobs[j].depth.format,
                                          image_import_form(jobs[j].depth.data, jobs[j].depth.row_stride, p.cols_d, jobs[j].depth.format)};
            ij.dst[kRoleDepth] = (unsigned char *)(c->alnb_up + w.up_at[u]);
            HIPCHK(c, launch_image_import(ij, st));
            HIPCHK(c, hipMemcpyAsync(pin_up + w.up_at[u], c->alnb_up + w.up_at[u], 2 * Pd, hipMemcpyDeviceToHost, st));
            any_dev = true;
        }
        if (any_dev) HIPCHK(c, wait_stream(st));
        char *pin_planes = pin_up + w.up_bytes;
        c->alnb_host_counts.assign(4 * (size_t)J, 0);
        for (int j = 0; j < J; ++j) {
            const tdlo_align_params &p = jobs[j].p;
            const tdlo_image_view hv{pin_up + w.up_at[w.up_of[j]], TDLO_IMG_U16C1, TDLO_MEM_HOST, 2ll * p.cols_d, nullptr};
            if (tdlo_align_depth_host(&hv, &p, (unsigned short *)(pin_planes + (w.plane_off[j] - w.plane_off[0])), &c->alnb_host_counts[4 * (size_t)j]))
                return fail(c, TDLO_E_INVALID, "align batch: the host statement refused a job");
        }
        HIPCHK(c, hipMemcpyAsync(arena + w.plane_off[0], pin_planes, plane_bytes, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipEventRecord(c->alnb_ev_up, st));
        c->alnb_up_pending = true;
        if ((size_t)w.scratch_bytes < c->alnb_armed) c->alnb_armed = (size_t)w.scratch_bytes;      // (planes of this layout may lie over words that were armed)
        c->aln_route[1] += J;
        return TDLO_OK;
    }
    c->alnb_host_counts.clear();
    // ---- the host views: packed into the pinned block, ONE copy
    {
        std::vector<char> done(w.up_at.size(), 0);
        for (int j = 0; j < J; ++j) {
            const int u = w.up_of[j];
            if (u < 0 || done[u]) continue;
            done[u] = 1;
            image_pack_host(&jobs[j].depth, jobs[j].p.rows_d, jobs[j].p.cols_d, pin_up + w.up_at[u]);
        }
        if (w.up_bytes) HIPCHK(c, hipMemcpyAsync(c->alnb_up, pin_up, w.up_bytes, hipMemcpyHostToDevice, st));
    }
    // ---- the table and the zeroed count words: one copy
    char *pin_tab = c->alnb_pin + kAlnbPinCounts;
    const size_t cnt_bytes = (size_t)(w.table_off - w.counts_off[0]);
    std::memset(pin_tab, 0, cnt_bytes);
    AlignBatchRec *h_tab = (AlignBatchRec *)(pin_tab + cnt_bytes);
    for (int j = 0; j < J; ++j) {
        AlignBatchRec &r = h_tab[j];
        std::memset(&r, 0, sizeof r);
        align_job(&jobs[j].depth, &jobs[j].p, r.job);
        if (!w.dev[j]) { r.job.depth = (const unsigned char *)(c->alnb_up + w.up_at[w.up_of[j]]); r.job.row_stride = 2ll * jobs[j].p.cols_d; r.job.format = TDLO_IMG_U16C1; }
        r.scratch = (unsigned *)(arena + w.scratch_off[j]);
        r.plane = (unsigned short *)(arena + w.plane_off[j]);
        r.counts = (unsigned long long *)(arena + w.counts_off[j]);
    }
    HIPCHK(c, hipMemcpyAsync(arena + w.counts_off[0], pin_tab, cnt_bytes + sizeof(AlignBatchRec) * (size_t)J, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(c->alnb_ev_up, st));
    c->alnb_up_pending = true;
    // ---- the scratch region: filled where it was not yet (a new arena, a region that grows); everything else of it is armed (the plan's invariant)
    const size_t armed = std::min(c->alnb_armed, (size_t)w.scratch_bytes);
    if (armed < (size_t)w.scratch_bytes) HIPCHK(c, hipMemsetAsync(arena + armed, 0xff, (size_t)w.scratch_bytes - armed, st));
    c->alnb_armed = 0;                                      // (a call that fails between its launches leaves offered words behind: filled again next time)
    unsigned long long *res = (unsigned long long *)c->alnb_pin;
    if (J >= align_batch_min(c)) {
        HIPCHK(c, launch_align_batch((const AlignBatchRec *)(arena + w.table_off), J, w.most_Pd, w.most_Pc, res, st));
        c->aln_route[2] += J;
    } else {
        for (int j = 0; j < J; ++j) HIPCHK(c, launch_align(h_tab[j].job, h_tab[j].scratch, h_tab[j].plane, h_tab[j].counts, res + 4 * j, st));
        c->aln_route[0] += J; c->aln_route[3] += J;
    }
    c->alnb_armed = (size_t)w.scratch_bytes;
    return TDLO_OK;
}

// after a wait of the context's stream that followed align_batch_enqueue: job j's four counts
static void align_batch_counts_fetch(const tdlo_ctx *c, int j, long long counts[4]) {
    for (int i = 0; i < 4; ++i)
        counts[i] = c->alnb_host_counts.empty() ? (long long)((const unsigned long long *)c->alnb_pin)[4 * j + i] : c->alnb_host_counts[4 * (size_t)j + i];
}

int tdlo_align_depth_batch(tdlo_ctx *c, const tdlo_align_job *jobs, int J, unsigned short *const *aligned_out, const unsigned short **device_planes,
                           long long *counts, int *rc_each) {
    if (!c) return TDLO_E_INVALID;
    AlignBatchWork w;
    std::vector<char> out_dev;
    int rc = align_batch_refusal(c, jobs, J, aligned_out, w, &out_dev);
    if (rc) return rc;
    std::vector<const unsigned short *> planes(J, nullptr);
    if ((rc = align_batch_enqueue(c, jobs, w, planes.data()))) { (void)hipStreamSynchronize(c->stream); return rc; }
    bool to_host = counts != nullptr;
    if (aligned_out)
        for (int j = 0; j < J; ++j) {
            if (!aligned_out[j]) continue;
            HIPCHK(c, hipMemcpyAsync(aligned_out[j], planes[j], 2 * (size_t)jobs[j].p.rows_c * jobs[j].p.cols_c, out_dev[j] ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
            to_host = to_host || !out_dev[j];
        }
    if (to_host) HIPCHK(c, wait_stream(c->stream));
    if (counts) for (int j = 0; j < J; ++j) align_batch_counts_fetch(c, j, counts + 4 * j);
    if (device_planes) std::copy(planes.begin(), planes.end(), device_planes);
    if (rc_each) std::fill(rc_each, rc_each + J, 0);
    return TDLO_OK;
}

// The (camera, frame) entries of an aligning rig call: what refuses them on their own, the cameras with a placeholder depth plane (what the rig call's own
// checks see before the planes exist), the distinct jobs
struct RigAlignWork {
    std::vector<tdlo_rig_camera> cams;                      // every entry's camera, its depth the placeholder, later the arena's plane
    std::vector<int> job_of;                                // entry -> distinct job
    std::vector<tdlo_align_job> jobs;                       // the distinct jobs
    AlignBatchWork w;
};
alignas(8) static const unsigned short kRigAlignPlaceholder[4] = {0, 0, 0, 0};

static int rig_align_entries(tdlo_ctx *c, const tdlo_rig_camera *cams, const tdlo_align_job *raw, int K, int rows, int cols, RigAlignWork &ra) {
    if (!cams || !raw || K < 1 || K > 64) return fail(c, TDLO_E_INVALID, "aligning rig: 1 .. 64 cameras and their raw depth");
    for (int k = 0; k < K; ++k) {
        if (cams[k].depth) return fail(c, TDLO_E_INVALID, "aligning rig: a camera brings a depth plane (cams[k].depth must be NULL: the plane comes from raw[k])");
        if (int rc = align_refusal(c, &raw[k].depth, &raw[k].p)) return rc;
        if (raw[k].p.rows_c != rows || raw[k].p.cols_c != cols) return fail(c, TDLO_E_INVALID, "aligning rig: the colour size of raw[k].p is not the rig's rows x cols");
        ra.cams.push_back(cams[k]);
        ra.cams.back().depth = kRigAlignPlaceholder;
    }
    return TDLO_OK;
}

// the distinct jobs of all entries (raw: one pointer per entry), checked as a batch
static int rig_align_jobs(tdlo_ctx *c, const std::vector<const tdlo_align_job *> &raw, RigAlignWork &ra) {
    const int E = (int)raw.size();
    std::vector<tdlo_image_view> v(E);
    std::vector<tdlo_align_params> p(E);
    for (int e = 0; e < E; ++e) { v[e] = raw[e]->depth; p[e] = raw[e]->p; }
    ra.job_of.assign(E, 0);
    const int Jd = align_distinct_jobs(v.data(), p.data(), E, ra.job_of.data());
    if (Jd > kAlignBatchMaxJobs) return fail(c, TDLO_E_INVALID, "aligning rig: more than 1024 distinct jobs");
    ra.jobs.resize(Jd);
    for (int e = E - 1; e >= 0; --e) ra.jobs[ra.job_of[e]] = *raw[e];
    return align_batch_refusal(c, ra.jobs.data(), Jd, nullptr, ra.w, nullptr);
}

// the planes enqueued, every entry's camera pointed at its job's plane
static int rig_align_enqueue(tdlo_ctx *c, RigAlignWork &ra) {
    std::vector<const unsigned short *> planes(ra.jobs.size(), nullptr);
    if (int rc = align_batch_enqueue(c, ra.jobs.data(), ra.w, planes.data())) { (void)hipStreamSynchronize(c->stream); return rc; }
    for (size_t e = 0; e < ra.cams.size(); ++e) ra.cams[e].depth = planes[ra.job_of[e]];
    c->aln_route[4] += (long long)ra.jobs.size();
    return TDLO_OK;
}

// after the rig call's own wait: one row per entry
static void rig_align_counts(tdlo_ctx *c, const RigAlignWork &ra, long long *counts) {
    if (!counts) return;
    (void)hipStreamSynchronize(c->stream);                  // (idle after a rig call that reached its kernels; a rig call that failed early may not have waited)
    for (size_t e = 0; e < ra.job_of.size(); ++e) align_batch_counts_fetch(c, ra.job_of[e], counts + 4 * e);
}

int tdlo_rig_to_cloud_aligning(tdlo_ctx *c, int slot, const tdlo_rig_camera *cams, const tdlo_align_job *raw, int K, int rows, int cols, double leaf_size,
                               double *X_out, int x_capacity, int *n_out, int *n_raw_out, long long *counts) {
    if (!c) return TDLO_E_INVALID;
    RigAlignWork ra;
    int rc = rig_align_entries(c, cams, raw, K, rows, cols, ra);
    if (rc) return rc;
    std::vector<BatchPlanes> where;
    if ((rc = rig_refusal(c, slot, ra.cams.data(), K, rows, cols, leaf_size, where))) return rc;
    std::vector<const tdlo_align_job *> entries(K);
    for (int k = 0; k < K; ++k) entries[k] = raw + k;
    if ((rc = rig_align_jobs(c, entries, ra)) || (rc = rig_align_enqueue(c, ra))) return rc;
    rc = tdlo_rig_to_cloud(c, slot, ra.cams.data(), K, rows, cols, leaf_size, X_out, x_capacity, n_out, n_raw_out);
    rig_align_counts(c, ra, counts);
    return rc;
}

int tdlo_tracker_frame_from_rig_aligning(tdlo_tracker *t, const tdlo_rig_camera *cams, const tdlo_align_job *raw, int K, int rows, int cols, double leaf_size,
                                         double d_vis, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext, int *n_out, int *n_raw_out,
                                         tdlo_stats *stats, long long *counts) {
    if (!t) return TDLO_E_INVALID;
    tdlo_ctx *c = t->ctx;
    if (t->geodesic_coord.size() != (size_t)t->M) return fail(c, TDLO_E_INVALID, "the tracker has no nodes / geodesic coordinates yet (tdlo_tracker_initialize_*)");
    if (t->painter_on) return fail(c, TDLO_E_INVALID, "a rig frame with the self-occlusion switch on: that test is one camera's");
    RigAlignWork ra;
    int rc = rig_align_entries(c, cams, raw, K, rows, cols, ra);
    if (rc) return rc;
    std::vector<BatchPlanes> where;
    if ((rc = rig_refusal(c, t->slot, ra.cams.data(), K, rows, cols, leaf_size, where))) return rc;
    if (const char *why = tracker_rig_painter_refusal(t, ra.cams.data(), K, rows, cols)) return fail(c, TDLO_E_INVALID, why);
    std::vector<const tdlo_align_job *> entries(K);
    for (int k = 0; k < K; ++k) entries[k] = raw + k;
    if ((rc = rig_align_jobs(c, entries, ra)) || (rc = rig_align_enqueue(c, ra))) return rc;
    rc = tdlo_tracker_frame_from_rig(t, ra.cams.data(), K, rows, cols, leaf_size, d_vis, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext, n_out, n_raw_out, stats);
    rig_align_counts(c, ra, counts);
    return rc;
}

int tdlo_tracker_frames_from_rig_aligning_batch(tdlo_tracker *const *trackers, int F, const tdlo_rig_raw_frame *frames, int rows, int cols, double leaf_size,
                                                double d_vis, int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext, int *n_out, int *n_raw_out,
                                                tdlo_stats *stats, int *rc_each, long long *counts) {
    if (!trackers || F < 1 || !trackers[0]) return TDLO_E_INVALID;
    tdlo_ctx *c = trackers[0]->ctx;
    if (const char *why = tracker_batch_refusal(trackers, F, false)) return fail(c, TDLO_E_INVALID, why);
    if (!frames) return fail(c, TDLO_E_INVALID, "null frames");
    for (int i = 0; i < F; ++i)
        if (trackers[i]->painter_on) return fail(c, TDLO_E_INVALID, "a rig frame with the self-occlusion switch on: that test is one camera's");
    RigAlignWork ra;
    std::vector<const tdlo_align_job *> entries;
    std::vector<size_t> first(F, 0);
    for (int i = 0; i < F; ++i) {
        first[i] = ra.cams.size();
        if (int rc = rig_align_entries(c, frames[i].cams, frames[i].raw, frames[i].K, rows, cols, ra)) return rc;
        for (int k = 0; k < frames[i].K; ++k) entries.push_back(frames[i].raw + k);
    }
    std::vector<tdlo_rig_frame> fr(F);
    for (int i = 0; i < F; ++i) fr[i] = tdlo_rig_frame{trackers[i]->slot, ra.cams.data() + first[i], frames[i].K};
    for (int i = 0; i < F; ++i)
        if (trackers[i]->rig_painter_K)
            if (const char *why = tracker_rig_painter_refusal(trackers[i], fr[i].cams, fr[i].K, rows, cols)) return fail(c, TDLO_E_INVALID, why);
    std::vector<std::vector<BatchPlanes>> where;
    int rc = rig_batch_refusal(c, fr.data(), F, rows, cols, leaf_size, where);
    if (rc) return rc;
    if ((rc = rig_align_jobs(c, entries, ra)) || (rc = rig_align_enqueue(c, ra))) return rc;
    rc = tdlo_tracker_frames_from_rig_batch(trackers, F, fr.data(), rows, cols, leaf_size, d_vis, visible_nodes, n_vis, visible_nodes_extended, n_vis_ext, n_out,
                                            n_raw_out, stats, rc_each);
    rig_align_counts(c, ra, counts);
    return rc;
}

// ---- ropes of one colour: one cloud dealt out among F slots (include/trackdlo_hip.h has the statement; tdlo_assign.hip the kernels) -------------------------
// what refuses a call as a whole, nullptr when nothing does
static const char *assign_refusal(const tdlo_ctx *c, int src_slot, const tdlo_assign_rope *ropes, int F, double d_max) {
    const int S = (int)c->slots.size();
    if (F < 1 || F > S) return "cloud assign: F < 1 or F > max_frames";
    if (F > kAssignMaxRopes) return "cloud assign: more than 2048 ropes";
    if (const char *why = assign_fault(ropes, F, d_max)) return why;
    if (src_slot < 0 || src_slot >= S) return "cloud assign: the context has no such source slot";
    for (int f = 0; f < F; ++f) {
        if (ropes[f].slot < 0 || ropes[f].slot >= S) return "cloud assign: the context has no such destination slot";
        if (ropes[f].slot == src_slot) return "cloud assign: the source slot is among the destinations";
        for (int j = 0; j < f; ++j) if (ropes[j].slot == ropes[f].slot) return "cloud assign: the destinations must be distinct";
    }
    return nullptr;
}

static size_t asg_pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// the split's growing buffers: dev_bytes of asg_dev, T minima (+ the ticket) of asg_state, armed, res_words of asg_res.  Shared by the split and the clustering
static int asg_reserve(tdlo_ctx *c, size_t dev_bytes, size_t T, size_t res_words) {
    if (dev_bytes > c->asg_dev_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->asg_dev) hipFree(c->asg_dev);
        c->asg_dev = nullptr; c->asg_dev_cap = 0;
        const size_t cap = (dev_bytes + (dev_bytes >> 2) + 4095) & ~(size_t)4095;
        HIPCHK(c, hipMalloc((void **)&c->asg_dev, cap));
        c->asg_dev_cap = cap;
    }
    if (T > c->asg_state_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->asg_state) hipFree(c->asg_state);
        c->asg_state = nullptr; c->asg_state_cap = 0;
        const size_t cap = (T + 1023) & ~(size_t)1023;
        HIPCHK(c, hipMalloc((void **)&c->asg_state, sizeof(unsigned long long) * (cap + 8)));
        c->asg_state_cap = cap; c->asg_armed = false;
    }
    if (!c->asg_armed) {
        std::vector<unsigned long long> init(c->asg_state_cap + 8, 0x7ff0000000000000ull);
        for (size_t i = c->asg_state_cap; i < c->asg_state_cap + 8; ++i) init[i] = 0ull;
        HIPCHK(c, hipMemcpy(c->asg_state, init.data(), sizeof(unsigned long long) * init.size(), hipMemcpyHostToDevice));
        c->asg_armed = true;
    }
    if (res_words > c->asg_res_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->asg_res) hipHostFree(c->asg_res);
        c->asg_res = nullptr; c->asg_res_cap = 0;
        const size_t cap = (res_words + 1023) & ~(size_t)1023;
        HIPCHK(c, hipHostMalloc((void **)&c->asg_res, sizeof(unsigned long long) * cap, hipHostMallocDefault));
        std::memset(c->asg_res, 0, sizeof(unsigned long long) * cap);
        c->asg_res_cap = cap; c->asg_epoch = 0;
    }
    return TDLO_OK;
}

// the ONE host wait of a split: until k_assign_scatter's last workgroup has raised the word to asg_epoch
static int asg_wait(tdlo_ctx *c) {
    auto t_chk = std::chrono::steady_clock::now();
    for (unsigned spins = 1;; ++spins) {
        if ((unsigned)__atomic_load_n(c->asg_res, __ATOMIC_ACQUIRE) == c->asg_epoch) break;
        if ((spins & 255u) == 0) {
            const auto now = std::chrono::steady_clock::now();
            if (std::chrono::duration<double, std::micro>(now - t_chk).count() > 500.0) {
                t_chk = now;
                const hipError_t e = hipStreamQuery(c->stream);
                if (e == hipSuccess) {
                    if ((unsigned)__atomic_load_n(c->asg_res, __ATOMIC_ACQUIRE) == c->asg_epoch) break;
                    c->asg_armed = false;
                    return fail(c, TDLO_E_HIP, "the stream drained, but the cloud split did not report");
                }
                if (e != hipErrorNotReady) { c->asg_armed = false; return fail(c, TDLO_E_HIP, std::string("stream: ") + hipGetErrorString(e)); }
            }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    return TDLO_OK;
}

// what a split left behind: off[F + 1] of the flat node list, the counts, and -- the pre-pass rode -- the T squared minima in pinned host memory (until the next split)
struct AssignRun { std::vector<int> off, n_each; int n = 0, n_unowned = 0; const double *mins = nullptr; };

// the split of checked arguments: two launches, one wait.  owner / owner_d2 (NULL or n entries) are copied out behind it
static int assign_run(tdlo_ctx *c, int src_slot, const tdlo_assign_rope *ropes, int F, double d_max, bool ride, int *owner, double *owner_d2, AssignRun &run) {
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if (c->cloud_pending >= 0 && (rc = flush_pending_cloud(c))) return rc;
    const int n = c->slots[src_slot].N0;
    run.off.assign((size_t)F + 1, 0); run.n_each.assign(F, 0); run.n = n; run.n_unowned = 0; run.mins = nullptr;
    for (int f = 0; f < F; ++f) run.off[f + 1] = run.off[f] + ropes[f].M;
    const int T = run.off[F];
    if (n <= 0) {      // nothing to deal out: every destination is the cloud of 0 points
        for (int f = 0; f < F; ++f) { Slot &d = c->slots[ropes[f].slot]; d.N0 = 0; d.sorted_valid = false; }
        return TDLO_OK;
    }
    for (int f = 0; f < F; ++f) if ((rc = ensure_points(c, c->slots[ropes[f].slot], n))) return rc;      // a rope may own every point
    int nwg, cpb;
    assign_geometry(n, &nwg, &cpb);
    const size_t o_dst = asg_pad16(sizeof(int) * ((size_t)F + 1)), o_Y = o_dst + asg_pad16(sizeof(double *) * (size_t)F), tab = o_Y + sizeof(double) * 3 * (size_t)T;
    const size_t o_own = asg_pad16(tab), o_g = o_own + asg_pad16(sizeof(int) * (size_t)n), o_cnt = o_g + sizeof(double) * (size_t)n;
    const size_t need = o_cnt + asg_pad16(sizeof(int) * (size_t)nwg * F);
    if ((rc = asg_reserve(c, need, (size_t)T, 1 + (size_t)F + (size_t)T))) return rc;
    // the pinned staging block: [off | dst | Yx | Yy | Yz], copied up once
    if ((rc = ensure_pin(c, (tab + 7) / 8 + 8))) return rc;
    char *hp = (char *)c->pin;
    std::memset(hp, 0, o_Y);
    int *hoff = (int *)hp;
    double **hdst = (double **)(hp + o_dst);
    double *hY = (double *)(hp + o_Y);
    assign_flatten(ropes, F, hoff, hY, hY + T, hY + 2 * (size_t)T);
    for (int f = 0; f < F; ++f) hdst[f] = c->slots[ropes[f].slot].Xraw;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->asg_dev, hp, tab, hipMemcpyHostToDevice, st));
    if (++c->asg_epoch == 0) ++c->asg_epoch;
    int *d_owner = (int *)(c->asg_dev + o_own);
    double *d_g = (double *)(c->asg_dev + o_g);
    ++c->asg_route[0];
    if (ride) ++c->asg_route[1];
    HIPCHK(c, launch_assign(c->slots[src_slot].Xraw, n, (const int *)c->asg_dev, (double *const *)(c->asg_dev + o_dst), (const double *)(c->asg_dev + o_Y), F, T,
                            d_max * d_max, d_owner, owner_d2 ? d_g : nullptr, (int *)(c->asg_dev + o_cnt), ride, c->asg_state, c->asg_state + c->asg_state_cap,
                            c->asg_res, c->asg_epoch, st));
    if ((rc = asg_wait(c))) return rc;
    long long owned = 0;
    for (int f = 0; f < F; ++f) {
        const int nf = (int)(unsigned)c->asg_res[1 + f];
        run.n_each[f] = nf; owned += nf;
        Slot &d = c->slots[ropes[f].slot];
        d.N0 = nf; d.sorted_valid = false;      // as tdlo_set_cloud leaves it (nf == 0: as a rig that kept no pixel leaves it)
    }
    run.n_unowned = (int)(n - owned);
    if (ride) run.mins = (const double *)(c->asg_res + 1 + F);
    if (owner || owner_d2) {
        if (owner) HIPCHK(c, hipMemcpyAsync(owner, d_owner, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
        if (owner_d2) HIPCHK(c, hipMemcpyAsync(owner_d2, d_g, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, wait_stream(st));
    }
    return TDLO_OK;
}

int tdlo_cloud_assign(tdlo_ctx *c, int src_slot, const tdlo_assign_rope *ropes, int F, double d_max, int *n_each, int *n_unowned, int *owner, double *owner_d2) {
    if (!c) return TDLO_E_INVALID;
    if (const char *why = assign_refusal(c, src_slot, ropes, F, d_max)) return fail(c, TDLO_E_INVALID, why);
    AssignRun run;
    if (const int rc = assign_run(c, src_slot, ropes, F, d_max, false, owner, owner_d2, run)) return rc;
    if (n_each) std::copy(run.n_each.begin(), run.n_each.end(), n_each);
    if (n_unowned) *n_unowned = run.n_unowned;
    return TDLO_OK;
}

// whether the pre-pass of these ropes may ride in the split: the context's switch, the pre-pass's own one-launch conditions
static bool assign_ride_ok(const tdlo_ctx *c, const tdlo_assign_rope *ropes, int F) {
    if (!c->assign_ride || !c->direct_in) return false;
    for (int f = 0; f < F; ++f) if (ropes[f].M > kAssignRideMaxNodes) return false;
    return true;
}

int tdlo_cloud_assign_visibility(tdlo_ctx *c, int src_slot, const tdlo_assign_rope *ropes, int F, double d_max, double visibility_threshold, double d_vis,
                                 const double *const *geodesic_coord, int *n_each, int *n_unowned, double *const *node_dist, int *const *visible_nodes, int *n_vis,
                                 int *const *visible_nodes_extended, int *n_vis_ext) {
    if (!c) return TDLO_E_INVALID;
    if (const char *why = assign_refusal(c, src_slot, ropes, F, d_max)) return fail(c, TDLO_E_INVALID, why);
    if (!geodesic_coord) return fail(c, TDLO_E_INVALID, "cloud assign: null geodesic_coord");
    for (int f = 0; f < F; ++f) if (!geodesic_coord[f]) return fail(c, TDLO_E_INVALID, "cloud assign: null geodesic_coord");
    const bool ride = assign_ride_ok(c, ropes, F);
    AssignRun run;
    if (const int rc = assign_run(c, src_slot, ropes, F, d_max, ride, nullptr, nullptr, run)) return rc;
    if (n_each) std::copy(run.n_each.begin(), run.n_each.end(), n_each);
    if (n_unowned) *n_unowned = run.n_unowned;
    auto row = [&](auto *const *p, int f) { return p ? p[f] : nullptr; };
    auto one = [&](int *p, int f) { return p ? p + f : nullptr; };
    for (int f = 0; f < F; ++f) {
        const int M = ropes[f].M;
        if (ride && run.mins)
            vis_threshold_and_fill(run.mins + run.off[f], M, visibility_threshold, d_vis, geodesic_coord[f], row(node_dist, f), row(visible_nodes, f), one(n_vis, f),
                                   row(visible_nodes_extended, f), one(n_vis_ext, f));
        else if (run.n_each[f] > 0) {
            if (const int rc = tdlo_visibility_prepass(c, ropes[f].slot, ropes[f].Y, M, visibility_threshold, d_vis, geodesic_coord[f], row(node_dist, f),
                                                       row(visible_nodes, f), one(n_vis, f), row(visible_nodes_extended, f), one(n_vis_ext, f))) return rc;
        } else {      // a rope that owns nothing: the pre-pass of a cloud without a point
            const std::vector<double> none((size_t)M, std::numeric_limits<double>::infinity());
            vis_threshold_and_fill(none.data(), M, visibility_threshold, d_vis, geodesic_coord[f], row(node_dist, f), row(visible_nodes, f), one(n_vis, f),
                                   row(visible_nodes_extended, f), one(n_vis_ext, f));
        }
    }
    return TDLO_OK;
}

int tdlo_tracker_frames_from_shared_cloud_batch(tdlo_tracker *const *trackers, int F, int src_slot, double d_max, double d_vis,
                                                int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext, int *n_each, tdlo_stats *stats, int *rc_each) {
    if (!trackers || F < 1 || !trackers[0]) return TDLO_E_INVALID;
    tdlo_ctx *c = trackers[0]->ctx;
    if (const char *why = tracker_batch_refusal(trackers, F, false)) return fail(c, TDLO_E_INVALID, why);
    const int M = trackers[0]->M;
    std::vector<tdlo_assign_rope> ropes(F);
    for (int i = 0; i < F; ++i) ropes[i] = tdlo_assign_rope{trackers[i]->slot, trackers[i]->Y.data(), M};
    if (const char *why = assign_refusal(c, src_slot, ropes.data(), F, d_max)) return fail(c, TDLO_E_INVALID, why);
    const bool ride = assign_ride_ok(c, ropes.data(), F);
    AssignRun run;
    if (const int rc = assign_run(c, src_slot, ropes.data(), F, d_max, ride, nullptr, nullptr, run)) return rc;
    if (n_each) std::copy(run.n_each.begin(), run.n_each.end(), n_each);
    std::vector<int> rcs(F, 0), who;
    std::vector<tdlo_tracker *> sub;
    std::vector<double> mins;      // the riders' squared minima, the trackers that go on one behind the other
    for (int i = 0; i < F; ++i) {
        if (run.n_each[i] == 0) { rcs[i] = TDLO_E_EMPTY; continue; }      // the rope owns no point: no cloud, the tracker is left as it is
        sub.push_back(trackers[i]); who.push_back(i);
        if (ride && run.mins) mins.insert(mins.end(), run.mins + run.off[i], run.mins + run.off[i] + M);
    }
    std::vector<tdlo_stats> st(2 * (size_t)F);
    std::memset(st.data(), 0, sizeof(tdlo_stats) * st.size());
    std::vector<int> nv(F, 0), ne(F, 0), vis((size_t)F * M, 0), ext((size_t)F * M, 0);
    if (!sub.empty()) {
        const int Fs = (int)sub.size();
        std::vector<int> snv(Fs, 0), sne(Fs, 0), svis((size_t)Fs * M, 0), sext((size_t)Fs * M, 0), src(Fs, 0);
        std::vector<tdlo_stats> sst(2 * (size_t)Fs);
        std::memset(sst.data(), 0, sizeof(tdlo_stats) * sst.size());
        const int brc = tracker_frame_batch_impl(sub.data(), Fs, d_vis, svis.data(), snv.data(), sext.data(), sne.data(), sst.data(), src.data(), nullptr, 0, 0,
                                                 (ride && run.mins) ? mins.data() : nullptr);
        bool sany = false;
        for (int r : src) sany = sany || r != 0;
        for (int k = 0; k < Fs; ++k) {
            const int i = who[k];
            rcs[i] = (brc && !sany) ? brc : src[k];
            nv[i] = snv[k]; ne[i] = sne[k];
            std::copy(&svis[(size_t)M * k], &svis[(size_t)M * k] + M, &vis[(size_t)M * i]);
            std::copy(&sext[(size_t)M * k], &sext[(size_t)M * k] + M, &ext[(size_t)M * i]);
            st[2 * (size_t)i] = sst[2 * (size_t)k]; st[2 * (size_t)i + 1] = sst[2 * (size_t)k + 1];
        }
    }
    if (visible_nodes) std::copy(vis.begin(), vis.end(), visible_nodes);
    if (visible_nodes_extended) std::copy(ext.begin(), ext.end(), visible_nodes_extended);
    if (n_vis) std::copy(nv.begin(), nv.end(), n_vis);
    if (n_vis_ext) std::copy(ne.begin(), ne.end(), n_vis_ext);
    if (stats) std::copy(st.begin(), st.end(), stats);
    if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
    for (int i = 0; i < F; ++i)
        if (rcs[i]) return (rcs[i] == TDLO_E_EMPTY && run.n_each[i] == 0) ? fail(c, TDLO_E_EMPTY, "the rope owns no point of the shared cloud: no cloud for this frame") : rcs[i];
    return TDLO_OK;
}

// ---- ropes that hide one another: the painter test over a cell of ropes (include/trackdlo_hip.h has the statement; tdlo_cell_painter_lane.h the lane,
// tdlo_cell_painter_host.cpp the host statement, tdlo_cell_painter.hip the kernels) ------------------------------------------------------------------------
// From this many flat nodes x cameras on, tdlo_tracker_frames_from_shared_cloud_occluded_batch hands the cell to the kernels; below it, it runs the host
// statement: the same sets.  MEASURED (scripts/gpu_cell_painter.py, profiles/cell_painter_ab.txt; the rule set beforehand: the smallest measured N K at and above
// which the kernels are faster on every measured line): the host statement wins at N K = 90, 180, 270 and 360 (0.139 against 0.122 ms at 360), the kernels at
// 540 (0.082 against 0.095 ms) and on every line above it, up to 4.19 against 540 ms at N K = 49 152.  TDLO_CELL_PAINTER_MIN=n, read when the context is
// made, overrides.
constexpr long long kCellPainterMin = 540;
static long long cell_painter_min(const tdlo_ctx *c) { return c->cell_painter_min >= 0 ? c->cell_painter_min : kCellPainterMin; }

// where the kernels' words of the cells of one call lie in cel_pin (valid until the next enqueue)
struct CellWords { std::vector<const unsigned *> seen, hidden; };

// One upload of [cell table | camera records | nodes | link words], the two launches; the words are in place once the stream has passed them.  The cells are
// checked (cell_painter_fault); nothing waits here
static int cell_painter_enqueue(tdlo_ctx *c, int C, const tdlo_cell *cells, int rows, int cols, CellWords &cw) {
    HIPCHK(c, hipSetDevice(c->device));
    size_t sumK = 0, sumN = 0, sumW = 0, sumKW = 0, sumKN = 0;
    int Kmax = 0, Nmax = 0;
    std::vector<int> Ns(C);
    for (int i = 0; i < C; ++i) {
        const int N = cell_painter_nodes(cells[i].ropes, cells[i].F), K = cells[i].K, W = (N + 31) / 32;
        Ns[i] = N;
        sumK += (size_t)K; sumN += (size_t)N; sumW += (size_t)W; sumKW += (size_t)K * W; sumKN += (size_t)K * N;
        Kmax = std::max(Kmax, K); Nmax = std::max(Nmax, N);
    }
    const size_t cams_off = sizeof(CellJob) * (size_t)C, y_off = cams_off + sizeof(PainterCam) * sumK, link_off = y_off + sizeof(double) * 3 * sumN;
    const size_t up = link_off + sizeof(unsigned) * sumW, recs_off = (up + 15) & ~(size_t)15, dev_bytes = recs_off + sizeof(CellRec) * sumKN;
    const size_t words_off = (up + 7) & ~(size_t)7, pin_bytes = words_off + sizeof(unsigned) * 2 * sumKW;
    hipStream_t st = c->stream;
    if (dev_bytes > c->cel_dev_cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->cel_dev) hipFree(c->cel_dev);
        c->cel_dev = nullptr; c->cel_dev_cap = 0;
        const size_t cap = (dev_bytes + (dev_bytes >> 2) + 4095) & ~(size_t)4095;
        HIPCHK(c, hipMalloc(&c->cel_dev, cap));
        c->cel_dev_cap = cap;
    }
    if (pin_bytes > c->cel_pin_cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->cel_pin) hipHostFree(c->cel_pin);
        c->cel_pin = nullptr; c->cel_pin_cap = 0;
        const size_t cap = (pin_bytes + (pin_bytes >> 2) + 4095) & ~(size_t)4095;
        HIPCHK(c, hipHostMalloc((void **)&c->cel_pin, cap, hipHostMallocDefault));
        std::memset(c->cel_pin, 0, cap);
        c->cel_pin_cap = cap;
    }
    char *pin = c->cel_pin, *dev = (char *)c->cel_dev;
    CellJob *tab = (CellJob *)pin;
    PainterCam *cams = (PainterCam *)(pin + cams_off);
    double *Yp = (double *)(pin + y_off);
    unsigned *link = (unsigned *)(pin + link_off), *words = (unsigned *)(pin + words_off);
    cw.seen.assign(C, nullptr); cw.hidden.assign(C, nullptr);
    size_t ik = 0, iy = 0, il = 0, iw = 0, ir = 0;
    for (int i = 0; i < C; ++i) {
        const tdlo_cell &q = cells[i];
        const int N = Ns[i], K = q.K, W = (N + 31) / 32;
        for (int k = 0; k < K; ++k) rig_painter_camera(q.cams[k], q.rig_to_cam ? q.rig_to_cam + 12 * (size_t)k : nullptr, cams[ik + k]);
        cell_painter_flatten(q.ropes, q.F, Yp + iy, Yp + iy + N, Yp + iy + 2 * (size_t)N, link + il);
        tab[i] = CellJob{(const double *)(dev + y_off) + iy, (const unsigned *)(dev + link_off) + il, (const PainterCam *)(dev + cams_off) + ik,
                         (CellRec *)(dev + recs_off) + ir, words + iw, words + iw + (size_t)K * W, N, K, q.dlo_pixel_width, 0};
        cw.seen[i] = words + iw; cw.hidden[i] = words + iw + (size_t)K * W;
        ik += (size_t)K; iy += 3 * (size_t)N; il += (size_t)W; iw += 2 * (size_t)K * W; ir += (size_t)K * N;
    }
    HIPCHK(c, hipMemcpyAsync(dev, pin, up, hipMemcpyHostToDevice, st));
    HIPCHK(c, launch_cell_painter((const CellJob *)dev, C, Kmax, Nmax, rows, cols, st));
    c->cel_route[0] += (long long)sumK;
    return TDLO_OK;
}

int tdlo_cell_occlusion_batch(tdlo_ctx *c, int C, const tdlo_cell *cells, int rows, int cols, int *visible_nodes, int *n_vis, unsigned *seen_words,
                              unsigned *hidden_words) {
    if (!c) return TDLO_E_INVALID;
    if (C < 1 || C > kCellPainterMaxCells || !cells || !visible_nodes || !n_vis)
        return fail(c, TDLO_E_INVALID, "tdlo_cell_occlusion_batch: 1 .. 1024 cells, visible_nodes and n_vis");
    int Mmax = 0;
    for (int i = 0; i < C; ++i) {
        const tdlo_cell &q = cells[i];
        if (const char *why = cell_painter_fault(q.ropes, q.F, q.cams, q.rig_to_cam, q.K, rows, cols, q.dlo_pixel_width)) return fail(c, TDLO_E_INVALID, why);
        for (int f = 0; f < q.F; ++f) Mmax = std::max(Mmax, q.ropes[f].M);
    }
    CellWords cw;
    int rc = cell_painter_enqueue(c, C, cells, rows, cols, cw);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int> vis;
    size_t iw = 0, row = 0;
    for (int i = 0; i < C; ++i) {
        const tdlo_cell &q = cells[i];
        const int N = cell_painter_nodes(q.ropes, q.F);
        const size_t KW = (size_t)q.K * ((N + 31) / 32);
        int off = 0;
        for (int f = 0; f < q.F; ++f, ++row) {
            const tdlo_cell_rope &r = q.ropes[f];
            cell_painter_verdict(cw.seen[i], cw.hidden[i], q.K, N, off, r.M, r.node_dist, r.visibility_threshold, vis);
            n_vis[row] = (int)vis.size();
            std::copy(vis.begin(), vis.end(), visible_nodes + row * (size_t)Mmax);
            off += r.M;
        }
        if (seen_words) std::copy(cw.seen[i], cw.seen[i] + KW, seen_words + iw);
        if (hidden_words) std::copy(cw.hidden[i], cw.hidden[i] + KW, hidden_words + iw);
        iw += KW;
    }
    return TDLO_OK;
}

// The shared-cloud tracker call with the cell's verdict in place of every tracker's visible set.  The cell is the F trackers' ropes in the call's order, the
// ones that own no point included (they hide others).  Kernel route: the two launches go in front of the split, whose one wait they share; host route: the
// statement is run on the host while nothing of the device is waited for.  Either way the words stand before the pre-pass's distances are thresholded
int tdlo_tracker_frames_from_shared_cloud_occluded_batch(tdlo_tracker *const *trackers, int F, int src_slot, double d_max, double d_vis, const tdlo_cell_view *view,
                                                         int *visible_nodes, int *n_vis, int *visible_nodes_extended, int *n_vis_ext, int *n_each, tdlo_stats *stats,
                                                         int *rc_each) {
    if (!trackers || F < 1 || !trackers[0]) return TDLO_E_INVALID;
    tdlo_ctx *c = trackers[0]->ctx;
    if (const char *why = tracker_batch_refusal(trackers, F, false)) return fail(c, TDLO_E_INVALID, why);
    if (!view) return fail(c, TDLO_E_INVALID, "frames_from_shared_cloud_occluded_batch: null view");
    const int M = trackers[0]->M;
    for (int i = 0; i < F; ++i)
        if (trackers[i]->painter_on || trackers[i]->rig_painter_K)
            return fail(c, TDLO_E_INVALID, "frames_from_shared_cloud_occluded_batch: a tracker has a self-occlusion switch on (the cell test subsumes both)");
    std::vector<tdlo_assign_rope> ropes(F);
    std::vector<tdlo_cell_rope> cr(F);
    for (int i = 0; i < F; ++i) {
        ropes[i] = tdlo_assign_rope{trackers[i]->slot, trackers[i]->Y.data(), M};
        cr[i] = tdlo_cell_rope{trackers[i]->Y.data(), M, nullptr, trackers[i]->visibility_threshold};
    }
    if (const char *why = assign_refusal(c, src_slot, ropes.data(), F, d_max)) return fail(c, TDLO_E_INVALID, why);
    if (const char *why = cell_painter_fault(cr.data(), F, view->cams, view->rig_to_cam, view->K, view->rows, view->cols, view->dlo_pixel_width, false))
        return fail(c, TDLO_E_INVALID, why);
    const int K = view->K, N = F * M, W = (N + 31) / 32;
    const bool kernels = (long long)N * K >= cell_painter_min(c);
    CellWords cw;
    std::vector<unsigned> hseen, hhidden;
    const unsigned *seen = nullptr, *hidden = nullptr;
    if (kernels) {
        const tdlo_cell cell{cr.data(), F, view->cams, view->rig_to_cam, K, view->dlo_pixel_width};
        if (const int rc = cell_painter_enqueue(c, 1, &cell, view->rows, view->cols, cw)) return rc;
        seen = cw.seen[0]; hidden = cw.hidden[0];
    }
    const bool ride = assign_ride_ok(c, ropes.data(), F);
    AssignRun run;
    if (const int rc = assign_run(c, src_slot, ropes.data(), F, d_max, ride, nullptr, nullptr, run)) {
        if (kernels) (void)hipStreamSynchronize(c->stream);      // (the words are not read; nothing of this call stays in flight)
        return rc;
    }
    if (kernels && run.n <= 0) HIPCHK(c, hipStreamSynchronize(c->stream));      // (a source of 0 points: the split launched nothing and waited for nothing)
    if (n_each) std::copy(run.n_each.begin(), run.n_each.end(), n_each);
    std::vector<int> rcs(F, 0), who;
    std::vector<tdlo_tracker *> sub;
    std::vector<double> mins;
    for (int i = 0; i < F; ++i) {
        if (run.n_each[i] == 0) { rcs[i] = TDLO_E_EMPTY; continue; }
        sub.push_back(trackers[i]); who.push_back(i);
        if (ride && run.mins) mins.insert(mins.end(), run.mins + run.off[i], run.mins + run.off[i] + M);
    }
    std::vector<tdlo_stats> st(2 * (size_t)F);
    std::memset(st.data(), 0, sizeof(tdlo_stats) * st.size());
    std::vector<int> nv(F, 0), ne(F, 0), vis((size_t)F * M, 0), ext((size_t)F * M, 0);
    if (!sub.empty()) {
        if (!kernels) {      // the host statement, on every rope of the cell
            std::vector<PainterCam> pc(K);
            for (int k = 0; k < K; ++k) rig_painter_camera(view->cams[k], view->rig_to_cam ? view->rig_to_cam + 12 * (size_t)k : nullptr, pc[k]);
            std::vector<double> xyz(3 * (size_t)N);
            std::vector<unsigned> link(W);
            hseen.assign((size_t)K * W, 0u); hhidden.assign((size_t)K * W, 0u);
            cell_painter_flatten(cr.data(), F, xyz.data(), xyz.data() + N, xyz.data() + 2 * (size_t)N, link.data());
            cell_painter_host(xyz.data(), xyz.data() + N, xyz.data() + 2 * (size_t)N, link.data(), N, pc.data(), K, view->rows, view->cols, view->dlo_pixel_width,
                              hseen.data(), hhidden.data());
            seen = hseen.data(); hidden = hhidden.data();
            c->cel_route[1] += K;
        }
        // (kernel route: the split's wait came after the two launches in stream order, so the words are in place)
        const std::function<void(int, const tdlo_tracker *, std::vector<int> &)> verdict = [&](int k, const tdlo_tracker *t, std::vector<int> &qv) {
            cell_painter_verdict(seen, hidden, K, N, who[k] * M, M, t->frame_dist.data(), t->visibility_threshold, qv);
        };
        const int Fs = (int)sub.size();
        std::vector<int> snv(Fs, 0), sne(Fs, 0), svis((size_t)Fs * M, 0), sext((size_t)Fs * M, 0), src(Fs, 0);
        std::vector<tdlo_stats> sst(2 * (size_t)Fs);
        std::memset(sst.data(), 0, sizeof(tdlo_stats) * sst.size());
        const int brc = tracker_frame_batch_impl(sub.data(), Fs, d_vis, svis.data(), snv.data(), sext.data(), sne.data(), sst.data(), src.data(), nullptr, 0, 0,
                                                 (ride && run.mins) ? mins.data() : nullptr, &verdict);
        bool sany = false;
        for (int r : src) sany = sany || r != 0;
        for (int k = 0; k < Fs; ++k) {
            const int i = who[k];
            rcs[i] = (brc && !sany) ? brc : src[k];
            nv[i] = snv[k]; ne[i] = sne[k];
            std::copy(&svis[(size_t)M * k], &svis[(size_t)M * k] + M, &vis[(size_t)M * i]);
            std::copy(&sext[(size_t)M * k], &sext[(size_t)M * k] + M, &ext[(size_t)M * i]);
            st[2 * (size_t)i] = sst[2 * (size_t)k]; st[2 * (size_t)i + 1] = sst[2 * (size_t)k + 1];
        }
    }
    if (visible_nodes) std::copy(vis.begin(), vis.end(), visible_nodes);
    if (visible_nodes_extended) std::copy(ext.begin(), ext.end(), visible_nodes_extended);
    if (n_vis) std::copy(nv.begin(), nv.end(), n_vis);
    if (n_vis_ext) std::copy(ne.begin(), ne.end(), n_vis_ext);
    if (stats) std::copy(st.begin(), st.end(), stats);
    if (rc_each) std::copy(rcs.begin(), rcs.end(), rc_each);
    for (int i = 0; i < F; ++i)
        if (rcs[i]) return (rcs[i] == TDLO_E_EMPTY && run.n_each[i] == 0) ? fail(c, TDLO_E_EMPTY, "the rope owns no point of the shared cloud: no cloud for this frame") : rcs[i];
    return TDLO_OK;
}

// ---- starting ropes of one colour: one cloud clustered into F slots (include/trackdlo_hip.h has the statement; tdlo_cluster.hip the kernels) ---------------------
// what refuses a call as a whole, nullptr when nothing does
static const char *cluster_refusal(const tdlo_ctx *c, int src_slot, const int *dst_slots, int F, double tol, int min_size) {
    const int S = (int)c->slots.size();
    if (F < 1 || F > S) return "cloud cluster: F < 1 or F > max_frames";
    if (F > kAssignMaxRopes) return "cloud cluster: more than 2048 destinations";
    if (!dst_slots) return "cloud cluster: null dst_slots";
    if (const char *why = cluster_fault(F, tol, min_size)) return why;
    if (src_slot < 0 || src_slot >= S) return "cloud cluster: the context has no such source slot";
    for (int f = 0; f < F; ++f) {
        if (dst_slots[f] < 0 || dst_slots[f] >= S) return "cloud cluster: the context has no such destination slot";
        if (dst_slots[f] == src_slot) return "cloud cluster: the source slot is among the destinations";
        for (int j = 0; j < f; ++j) if (dst_slots[j] == dst_slots[f]) return "cloud cluster: the destinations must be distinct";
    }
    if (c->slots[src_slot].N0 > kClusterMaxPoints) return "cloud cluster: more than 262 144 points (every pair is tested: a call's time must stay bounded)";
    return nullptr;
}

struct ClusterRun { std::vector<int> n_each; int n = 0, n_clusters = 0, n_unowned = 0; };

// the clustering of checked arguments.  Device route: the cluster launches and k_assign_scatter, ONE wait.  Host route (TDLO_CLUSTER=host, or a lane gave up): the
// cloud comes down, owners and their per-workgroup counts go up, the same k_assign_scatter.  owner (NULL or n entries) is copied out behind it
static int cluster_run(tdlo_ctx *c, int src_slot, const int *dst_slots, int F, double tol, int min_size, int *owner, ClusterRun &run) {
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if (c->cloud_pending >= 0 && (rc = flush_pending_cloud(c))) return rc;
    const int n = c->slots[src_slot].N0;
    run.n_each.assign(F, 0); run.n = n; run.n_clusters = 0; run.n_unowned = 0;
    if (n <= 0) {      // nothing to cluster: every destination is the cloud of 0 points
        for (int f = 0; f < F; ++f) { Slot &d = c->slots[dst_slots[f]]; d.N0 = 0; d.sorted_valid = false; }
        return TDLO_OK;
    }
    for (int f = 0; f < F; ++f) if ((rc = ensure_points(c, c->slots[dst_slots[f]], n))) return rc;      // a cluster may hold every point
    int nwg, cpb;
    assign_geometry(n, &nwg, &cpb);
    const size_t chunks = ((size_t)n + kBlock - 1) / kBlock, ints = asg_pad16(sizeof(int) * (size_t)n);
    // asg_dev: [dst x F | owner | counts] -- what the host route sends up in one copy -- then [parent | size | rank | kept roots per chunk]
    const size_t o_own = asg_pad16(sizeof(double *) * (size_t)F), o_cnt = o_own + ints, o_par = o_cnt + asg_pad16(sizeof(int) * (size_t)nwg * F);
    const size_t o_size = o_par + ints, o_rank = o_size + ints, o_kc = o_rank + ints, need = o_kc + asg_pad16(sizeof(int) * chunks);
    if ((rc = asg_reserve(c, need, 1, 1 + (size_t)F + 2)) || (rc = ensure_pin(c, o_par / 8 + 8))) return rc;
    char *hp = (char *)c->pin;
    double **hdst = (double **)hp;
    for (int f = 0; f < F; ++f) hdst[f] = c->slots[dst_slots[f]].Xraw;
    hipStream_t st = c->stream;
    const double *X = c->slots[src_slot].Xraw;
    int *d_owner = (int *)(c->asg_dev + o_own), *d_cnt = (int *)(c->asg_dev + o_cnt);
    unsigned long long *giveup = c->asg_res + 1 + F, *n_clusters = giveup + 1;      // behind the scatter's [word | F counts]
    auto scatter = [&]() {
        if (++c->asg_epoch == 0) ++c->asg_epoch;
        return launch_assign_scatter(X, n, d_owner, d_cnt, nullptr, (double *const *)c->asg_dev, nullptr, F, 0, false, c->asg_state, c->asg_state + c->asg_state_cap,
                                     c->asg_res, c->asg_epoch, st);
    };
    bool host = c->cluster_host;
    if (!host) {
        __atomic_store_n(giveup, 0ull, __ATOMIC_RELEASE);
        HIPCHK(c, hipMemcpyAsync(c->asg_dev, hp, sizeof(double *) * (size_t)F, hipMemcpyHostToDevice, st));
        HIPCHK(c, launch_cluster(X, n, tol * tol, min_size, F, (int *)(c->asg_dev + o_par), (int *)(c->asg_dev + o_size), (int *)(c->asg_dev + o_rank),
                                 (int *)(c->asg_dev + o_kc), d_owner, d_cnt, giveup, n_clusters, st));
        HIPCHK(c, scatter());
        if ((rc = asg_wait(c))) return rc;
        if (__atomic_load_n(giveup, __ATOMIC_ACQUIRE)) host = true;      // a lane ran out of attempts: what the launches wrote is overwritten below
        else { run.n_clusters = (int)(unsigned)*n_clusters; ++c->clu_route[0]; }
    }
    if (host) {
        std::vector<double> Xh(3 * (size_t)n);
        HIPCHK(c, hipMemcpyAsync(Xh.data(), X, sizeof(double) * Xh.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(c, wait_stream(st));
        int *h_owner = (int *)(hp + o_own);
        if (!cluster_owners_host(Xh.data(), n, F, tol * tol, min_size, h_owner, &run.n_clusters)) return fail(c, TDLO_E_NUMERIC, "cloud cluster: the host statement gave up");
        cluster_counts_host(h_owner, n, F, kBlock, nwg, cpb, (int *)(hp + o_cnt));
        HIPCHK(c, hipMemcpyAsync(c->asg_dev, hp, o_par, hipMemcpyHostToDevice, st));
        HIPCHK(c, scatter());
        if ((rc = asg_wait(c))) return rc;
        ++c->clu_route[1];
    }
    long long owned = 0;
    for (int f = 0; f < F; ++f) {
        const int nf = (int)(unsigned)c->asg_res[1 + f];
        run.n_each[f] = nf; owned += nf;
        Slot &d = c->slots[dst_slots[f]];
        d.N0 = nf; d.sorted_valid = false;      // as tdlo_set_cloud leaves it
    }
    run.n_unowned = (int)(n - owned);
    if (owner) {
        HIPCHK(c, hipMemcpyAsync(owner, d_owner, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, wait_stream(st));
    }
    return TDLO_OK;
}

int tdlo_cloud_cluster(tdlo_ctx *c, int src_slot, const int *dst_slots, int F, double tol, int min_size, int *n_clusters, int *n_each, int *n_unowned, int *owner) {
    if (!c) return TDLO_E_INVALID;
    if (const char *why = cluster_refusal(c, src_slot, dst_slots, F, tol, min_size)) return fail(c, TDLO_E_INVALID, why);
    ClusterRun run;
    if (const int rc = cluster_run(c, src_slot, dst_slots, F, tol, min_size, owner, run)) return rc;
    if (n_clusters) *n_clusters = run.n_clusters;
    if (n_each) std::copy(run.n_each.begin(), run.n_each.end(), n_each);
    if (n_unowned) *n_unowned = run.n_unowned;
    return TDLO_OK;
}

int tdlo_tracker_initialize_from_shared_cloud_batch(tdlo_tracker *const *trackers, int F, int src_slot, double tol, int min_size, double mu, int max_iter,
                                                    double *sigma2_out, int *n_clusters, int *n_each, int *rc_each) {
    if (!trackers || F < 1 || !trackers[0]) return TDLO_E_INVALID;
    tdlo_ctx *c = trackers[0]->ctx;
    const int M = trackers[0]->M;
    if (F > (int)c->slots.size()) return fail(c, TDLO_E_INVALID, "initialize_from_shared_cloud_batch: more trackers than the context has slots");
    std::vector<int> slots(F);
    for (int i = 0; i < F; ++i) {      // (what tdlo_tracker_initialize_from_cloud_batch would refuse behind the split is refused in front of it)
        const tdlo_tracker *t = trackers[i];
        if (!t) return fail(c, TDLO_E_INVALID, "initialize_from_shared_cloud_batch: a tracker is null");
        if (t->ctx != c) return fail(c, TDLO_E_INVALID, "initialize_from_shared_cloud_batch: the trackers of a batch share one context");
        if (t->M != M) return fail(c, TDLO_E_INVALID, "initialize_from_shared_cloud_batch: the trackers of a batch share num_of_nodes");
        slots[i] = t->slot;
    }
    if (M < 4 || M > reg_max_nodes()) return fail(c, TDLO_E_INVALID, "initialize_from_shared_cloud_batch: a tracker has 4 .. " + std::to_string(reg_max_nodes()) + " nodes (tdlo_reg)");
    if (max_iter < 0 || !(mu >= 0 && mu < 1)) return fail(c, TDLO_E_INVALID, "initialize_from_shared_cloud_batch: bad reg arguments");
    if (const char *why = cluster_refusal(c, src_slot, slots.data(), F, tol, min_size)) return fail(c, TDLO_E_INVALID, why);
    ClusterRun run;
    if (const int rc = cluster_run(c, src_slot, slots.data(), F, tol, min_size, nullptr, run)) return rc;
    if (n_clusters) *n_clusters = run.n_clusters;
    if (n_each) std::copy(run.n_each.begin(), run.n_each.end(), n_each);
    if (run.n_clusters != F)
        return fail(c, TDLO_E_INVALID, "initialize_from_shared_cloud_batch: the cloud has " + std::to_string(run.n_clusters) + " clusters for " + std::to_string(F) +
                                           " trackers (the slots hold the split, no tracker was touched)");
    return tdlo_tracker_initialize_from_cloud_batch(trackers, F, mu, max_iter, sigma2_out, rc_each);
}

// The rope tdlo_tracker_render_result draws: the projection matrix it chooses and the reference's not_self_occluded_nodes.  false: no matrix to be had.
static bool tracker_render_rope(const tdlo_tracker *t, const double *proj, double pj[12], std::vector<int> &vis) {
    const int M = t->M;
    std::fill(pj, pj + 12, 0.0);
    if (proj) std::copy(proj, proj + 12, pj);
    else if (t->painter_on) std::copy(t->painter_proj, t->painter_proj + 12, pj);
    else if (t->frame_seen) { pj[0] = t->frame_cam[0]; pj[2] = t->frame_cam[2]; pj[5] = t->frame_cam[1]; pj[6] = t->frame_cam[3]; pj[10] = 1.0; }
    else return false;
    vis.clear();
    if (t->painter_on && t->frame_Y0.size() == 3 * (size_t)M) {
        const std::vector<double> zero(M, 0.0);
        self_occlusion_visible(t->frame_Y0.data(), M, t->painter_proj, t->painter_width, zero.data(), std::numeric_limits<double>::infinity(), vis);
    } else { vis.resize(M); for (int m = 0; m < M; ++m) vis[m] = m; }
    return true;
}

// The picture of the tracker's current nodes over the last colour frame (trackdlo_node.cpp:377-452).  vis = the reference's not_self_occluded_nodes (:401):
// the nodes the self-occlusion test leaves when no node is too far from the cloud, formed from the nodes the frame STARTED from (:279-343 run before
// tracking_step); every node when the test is off.  Reads the tracker, changes nothing of it.
int tdlo_tracker_render_result(tdlo_tracker *t, const double *proj, const tdlo_render_params *p, unsigned char *image_out, int corners[4]) {
    if (!t) return TDLO_E_INVALID;
    tdlo_ctx *c = t->ctx;
    const int M = t->M;
    double pj[12] = {0};
    std::vector<int> vis;
    if (!tracker_render_rope(t, proj, pj, vis))
        return fail(c, TDLO_E_INVALID, "tdlo_tracker_render_result: no projection matrix (none given, no tdlo_tracker_set_self_occlusion, no frame call yet)");
    return tdlo_render_result(c, nullptr, nullptr, c->last_col_rows, c->last_col_cols, t->Y.data(), M, pj, vis.data(), (int)vis.size(), p, image_out, corners);
}

// Rope i = tracker i's current nodes over image image_of[i], drawn by tdlo_render_result_batch.  Reads the trackers, changes nothing of them.
int tdlo_tracker_render_result_batch(tdlo_tracker *const *trackers, int F, const tdlo_render_image *images, int K, int rows, int cols, const int *image_of,
                                     const double *const *proj_each, const tdlo_render_params *const *params_each, int *corners) {
    if (!trackers || F < 1 || !trackers[0]) return TDLO_E_INVALID;
    tdlo_ctx *c = trackers[0]->ctx;
    if (F > 1024 || !image_of) return fail(c, TDLO_E_INVALID, "tdlo_tracker_render_result_batch: 1 .. 1024 trackers and an image for each");
    std::vector<tdlo_render_rope> ropes(F);
    std::vector<std::vector<int>> vis(F);
    std::vector<double> pj(12 * (size_t)F);
    for (int i = 0; i < F; ++i) {
        const tdlo_tracker *t = trackers[i];
        if (!t || t->M < 1 || t->Y.size() != 3 * (size_t)t->M)
            return fail(c, TDLO_E_INVALID, "tdlo_tracker_render_result_batch: tracker " + std::to_string(i) + " has no nodes");
        if (t->ctx != c) return fail(c, TDLO_E_INVALID, "tdlo_tracker_render_result_batch: tracker " + std::to_string(i) + " belongs to another context: the trackers of a batch share one");
        if (!tracker_render_rope(t, proj_each ? proj_each[i] : nullptr, pj.data() + 12 * (size_t)i, vis[i]))
            return fail(c, TDLO_E_INVALID, "tdlo_tracker_render_result_batch: tracker " + std::to_string(i) + ": no projection matrix (none given, no tdlo_tracker_set_self_occlusion, "
                                           "no frame call yet)");
        ropes[i] = tdlo_render_rope{image_of[i], t->M, t->Y.data(), pj.data() + 12 * (size_t)i, vis[i].data(), (int)vis[i].size(), params_each ? params_each[i] : nullptr};
    }
    return tdlo_render_result_batch(c, images, K, rows, cols, ropes.data(), F, corners);
}

// trackdlo_node.cpp:279-343 on the host (tdlo_host.cpp, self_occlusion_visible): O(M^2) integer tests, no kernel warranted
int tdlo_self_occlusion_visible(const double *Y, int M, const double proj[12], int dlo_pixel_width, const double *node_dist, double visibility_threshold,
                                int *visible_nodes, int *n_vis) {
    if (!Y || !proj || !node_dist || !visible_nodes || !n_vis || M < 1 || dlo_pixel_width < 1) return TDLO_E_INVALID;
    std::vector<int> v;
    self_occlusion_visible(Y, M, proj, dlo_pixel_width, node_dist, visibility_threshold, v);
    *n_vis = (int)v.size();
    std::copy(v.begin(), v.end(), visible_nodes);
    return TDLO_OK;
}

// trackdlo_node.cpp:345-360
int tdlo_extend_visible_nodes(const int *visible_nodes, int n_vis, const double *geodesic_coord, double d_vis, int *visible_nodes_extended, int *n_vis_ext) {
    if (n_vis < 0 || (n_vis > 0 && (!visible_nodes || !geodesic_coord)) || !visible_nodes_extended || !n_vis_ext) return TDLO_E_INVALID;
    std::vector<int> v(visible_nodes, visible_nodes + n_vis), e;
    std::sort(v.begin(), v.end());                                  // :346
    fill_visible_gaps(v, geodesic_coord, d_vis, e);
    *n_vis_ext = (int)e.size();
    std::copy(e.begin(), e.end(), visible_nodes_extended);
    return TDLO_OK;
}

int tdlo_tracker_set_self_occlusion(tdlo_tracker *t, const double *proj, int dlo_pixel_width) {
    if (!t) return TDLO_E_INVALID;
    if (!proj) { t->painter_on = false; return TDLO_OK; }
    if (dlo_pixel_width < 1) return fail(t->ctx, TDLO_E_INVALID, "tdlo_tracker_set_self_occlusion: dlo_pixel_width >= 1");
    std::copy(proj, proj + 12, t->painter_proj);
    t->painter_width = dlo_pixel_width; t->painter_on = true;
    return TDLO_OK;
}

}  // extern "C"
