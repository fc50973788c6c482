/* sageicp.h — C ABI of libsageicp_hip.so: the MI355X (gfx950) implementation of SAGE-ICP's
 * per-scan registration hot path.  Plain pointers and sizes only; no Eigen/Sophus/torch types.
 *
 * Every entry point below is what a binding of the reference's C++ interface for this path
 * would call; the reference interface each one replaces is cited as file:line relative to
 * NeSC-IV/sage-icp @ 2024_10_08, directory cpp/sage_icp/.  INTEGRATION.md shows the header
 * shim (sage-icp_amd/shim/sage_icp/core/{VoxelHashMap,Registration}.hpp) that keeps the
 * reference's C++ signatures on top of this ABI so ros/ros2/OdometryServer.cpp and
 * pipeline/sageICP.cpp compile unchanged.
 *
 * Conventions
 *   points   double[n][4] row-major = (x, y, z, label); identical to the memory of
 *            std::vector<Eigen::Vector4d>::data().
 *   pose     double[7] = (qx, qy, qz, qw, tx, ty, tz); identical to Sophus::SE3d::data().
 *   return   0 on success, negative on error (never throws); sageicp_last_error() gives text.
 *   threads  one call at a time per map handle (the reference's single ROS executor thread,
 *            ros/ros2/OdometryServer.cpp:356).  Different handles may be used concurrently.
 *   device   the HIP path is the only path: without a gfx950 device every compute entry
 *            returns SAGEICP_ERR_NO_DEVICE.  There is no CPU fallback in this library.
 *   NaN/Inf  the reference turns coordinates into voxel indices and labels into classes with
 *            static_cast<int> (VoxelHashMap.cpp:52-54,87-88,165; Preprocessing.cpp:58-64): undefined
 *            for values that are not finite, so there is no behaviour to reproduce.  Every entry that
 *            would cast one — AddPoints / Update (host and device), GetCorrespondences, RegisterFrame
 *            (host buffer or resident frame), VoxelDownsample, the pipeline — refuses the WHOLE call
 *            with SAGEICP_ERR_INVALID and changes nothing.  Where the reference IS defined it is
 *            followed: Preprocess() drops a point whose norm is not finite (both range tests fail,
 *            Preprocessing.cpp:176-177) — so the pipeline drops such points like the reference and only
 *            refuses non-finite LABELS —, TransformPoints and AlignClouds propagate NaN.
 */
#ifndef SAGEICP_H_
#define SAGEICP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAGEICP_OK 0
#define SAGEICP_ERR_INVALID (-1)    /* bad argument */
#define SAGEICP_ERR_NO_DEVICE (-2)  /* no usable gfx950 device / HIP runtime failure at init */
#define SAGEICP_ERR_HIP (-3)        /* a HIP call failed */
#define SAGEICP_ERR_RCCL (-4)       /* RCCL could not be loaded or a collective failed */
#define SAGEICP_ERR_CAPACITY (-5)   /* > 2^24 voxels, > 255 points per voxel, > 2^26 point slots, or a voxel
                                     * index beyond +-2^20 */

typedef struct sageicp_map sageicp_map;       /* opaque: host map + device mirror + scratch */
typedef struct sageicp_frame sageicp_frame;   /* opaque: a scan resident in HBM */
typedef struct sageicp_comm sageicp_comm;     /* opaque: RCCL communicator for query sharding */

/* Version of this header's ABI; sageicp_abi_version() returns the library's.  A binding must refuse
 * a library whose version differs (the header shim and the Python loader do): struct layouts
 * below are part of it.   2: sageicp_stats without the three fields that had become constant
 * zeros (us_group, us_gn, resorts), with pairs_evaluated / lanes_per_query / compact_scan;
 * capacity limits 2^24 voxels / 2^26 point slots (sageicp_map_point_slots) / |voxel index| < 2^20 (SAGEICP_ERR_CAPACITY);
 * sageicp_comm_describe, sageicp_map_pointcloud served from the HBM copy, sageicp_map_point_slots
 * (size-classed voxel storage).   3: sageicp_stats names its loop form (single_launch in the slot of
 * reserved0), sageicp_pipeline_prefetch_wait, non-finite input refused (SAGEICP_ERR_INVALID) at every entry
 * that would cast it.   4: sageicp_map_loop_status, sageicp_reload_env; then the dynamic vehicle filter —
 * sageicp_preprocess_dynamic, sageicp_cluster_emission_order, sageicp_dynfilter_info and the pipeline's
 * sageicp_pipeline_set_dynamic_vehicle_filter / sageicp_pipeline_dynamic_filter_info; then frames in device memory —
 * sageicp_device_frame, SAGEICP_DTYPE_*, sageicp_pipeline_register_frame_device, sageicp_frame_from_device; then outputs
 * in device memory — sageicp_device_points, sageicp_pipeline_source, sageicp_pipeline_source_device,
 * sageicp_map_pointcloud_device; then key-frame selection — sageicp_occupancy_params, sageicp_key_frame_info,
 * sageicp_pipeline_set_key_frames, sageicp_pipeline_key_frame_reset / _info / _grid / _grid_device,
 * sageicp_occupancy_grid, sageicp_occupancy_grid_device; then PointCloud2 payloads — sageicp_msg_layout, sageicp_msg_colors,
 * SAGEICP_MSG_*, sageicp_pipeline_register_frame_msg / _msg_device, sageicp_pipeline_source_msg / _msg_device,
 * sageicp_map_pointcloud_msg / _msg_device, sageicp_msg_output_fields; then correspondences of a device frame —
 * sageicp_get_correspondences_device; then the registration quality report — sageicp_quality,
 * sageicp_registration_quality / _device, sageicp_pipeline_set_quality, sageicp_pipeline_quality; then a batch of
 * candidate poses and relocalisation — sageicp_pose_score, sageicp_score_poses / _device, sageicp_relocalize_params,
 * sageicp_relocalize_info, sageicp_relocalize_candidates, sageicp_relocalize / _device; then the archive of a map —
 * sageicp_archive_info, sageicp_archive_voxel, SAGEICP_ARCHIVE_* / SAGEICP_SESSION, sageicp_map_set_archive,
 * sageicp_map_archive_info / _clear / _voxels / _rows / _rows_device / _msg / _msg_device, sageicp_pipeline_set_archive;
 * then recall — sageicp_recall_info, sageicp_map_recall, sageicp_pipeline_recall; then loop closure —
 * sageicp_closure_info, sageicp_closure_corrections, sageicp_map_session_stays, sageicp_map_session_corrected / _device,
 * sageicp_pipeline_closure, sageicp_pipeline_session_corrected / _device; then the session rebuild —
 * sageicp_rebuild_info, sageicp_map_session_rebuild, sageicp_pipeline_session_rebuild
 * (additions only: no existing struct or entry changed). */
#define SAGEICP_ABI_VERSION 4

/* Filled by sageicp_register_frame*.  Times are microseconds. */
typedef struct sageicp_stats {
    int32_t iterations;         /* ICP iterations executed (<= 500, Registration.cpp:96) */
    int32_t converged;          /* 1 if ||log(est)|| < 1e-4 ended the loop (Registration.cpp:137) */
    uint64_t n_queries;         /* points of the frame (this rank's shard) */
    uint64_t n_corr_first;      /* accepted correspondences, first iteration (all ranks) */
    uint64_t n_corr_last;       /* accepted correspondences, last iteration (all ranks) */
    double last_step_norm;      /* ||log(est)|| of the last iteration */
    double us_wall;             /* host wall time of the call */
    double us_upload;           /* frame H2D + lazy map-mirror refresh inside the call */
    /* device time per kernel summed over the executed iterations (HIP events on the launch
     * stream); filled only when profiling is enabled with sageicp_set_profiling(). */
    double us_nn;               /* k_icp: pose apply + correspondence search + Gauss-Newton sums */
    double us_fin;              /* k_fin: reduction of the partials, solve, pose update */
    uint32_t nn_launches;       /* k_icp launches that were timed (us_nn / nn_launches = mean duration) */
    uint32_t single_launch;     /* 1: the whole loop ran inside one launch (k_loop: a frame that fits the machine, one GPU) */
    uint64_t sum_candidates;    /* sum over iterations and queries of C_q: map points stored in the
                                 * <=27 existing neighbour voxels of each query (this rank) */
    uint32_t n_corr_hist[64];   /* accepted correspondences of the first 64 iterations */
    uint64_t pairs_evaluated;   /* (query, map point) pairs the search actually evaluated, all
                                 * iterations: sum_candidates minus what the cell lower bound pruned */
    uint32_t lanes_per_query;   /* lanes that shared one query in the search kernel (1..16) */
    uint32_t compact_scan;      /* 1: the search scanned the 16-B compact copy of the map behind its fp32
                                 * filter (big frames, dense voxels); 0: the full fp64 records */
} sageicp_stats;

/* ---- library ------------------------------------------------------------------------ */
int sageicp_abi_version(void);
const char *sageicp_last_error(void);
int sageicp_device_count(void);               /* number of visible HIP devices (0: none) */
void sageicp_set_profiling(int level);        /* 0 off; 1 HIP events around k_icp in one iteration
                                               * out of 8; 2 around every kernel of every iteration */
void sageicp_reload_env(void);                /* the SAGEICP_* tuning knobs are read from the environment once per process (at
                                               * first use, all together); this reads them again for the calls that begin
                                               * afterwards: a call in flight keeps the values it began with.  Not while
                                               * another thread changes the environment. */
void sageicp_set_counting(int on);            /* 1 (default): a call given a sageicp_stats counts C_q and the pairs it
                                               * evaluates (sum_candidates, pairs_evaluated: ~3 % of the search);
                                               * 0: those two fields stay zero, the others are filled as before.
                                               * A call without stats (the C++ shim's) never counts. */

/* ---- map: sage_icp::VoxelHashMap (core/VoxelHashMap.hpp:35-107) ------------------------ */
/* ctor, VoxelHashMap.hpp:79-88.  device: HIP device ordinal that will hold the mirror. */
sageicp_map *sageicp_map_create(double voxel_size, double max_distance,
                                int basic_points_per_voxel, int critical_points_per_voxel,
                                const int *basic_parts_labels, int n_labels, int device);
void sageicp_map_destroy(sageicp_map *map);
/* Single-process multi-GPU mode: the map spans `n` (1..8) devices — a full copy per device, every
 * mutation applied to all of them — and sageicp_register_frame[_resident] shards the frame over
 * them (contiguous blocks, one host thread and stream per device; the Gauss-Newton sums meet in
 * peer-mapped exchange blocks), so the unchanged caller of sage_icp::RegisterFrame() — the ROS2
 * node's single executor thread, ros/ros2/OdometryServer.cpp:104,356 — uses several GPUs.
 * devices[0] is rank 0 (where a resident frame and the pipeline's buffers live).  The
 * environment variable SAGEICP_DEVICES=0,1,2,3 applies the same to every map the process creates. */
int sageicp_map_set_devices(sageicp_map *map, const int *devices, int n);
int sageicp_map_num_devices(const sageicp_map *map);
/* Reference-order mode (off by default; the map must be empty when it is switched).  The search never
 * depends on the iteration order of the reference's tsl::robin_map (core/VoxelHashMap.hpp:106), but two
 * things a caller can observe do: RemovePointsFarFromLocation erases WHILE iterating the container
 * (VoxelHashMap.cpp:176-184), so the voxel that the backward-shift deletion moves into the bucket just
 * erased is skipped and survives until a later frame, and Pointcloud() lists the voxels in bucket order
 * (:132-142).  By default this library removes every far voxel and lists block-pool order.  With the
 * mode on, the map also keeps the bucket array the reference's container would have (robin_map v1.0.1:
 * growth from zero buckets at load 0.5, robin-hood displacement, backward-shift deletion, clear() keeps
 * the array, the reference's 20-bit VoxelHash) and both behaviours are the reference's.  Such a map is
 * maintained on the host (sageicp_map_update_pose_device and the pipeline fall back to the host update:
 * ~3 ms instead of ~0.3 ms per streamed frame).  SAGEICP_MAP_REFERENCE_ORDER=1 applies the mode to every
 * map the process creates (for callers behind the header shim).
 * sageicp_map_reference_order: 0 off; 1 on; -1 on, but an insertion met a probe distance the emulation
 * does not model (>= 128: not before a map holds several 10^5 voxels, where the reference's own table
 * degenerates with its 20-bit hash) — the map works, its order is no longer claimed to be the
 * reference's. */
int sageicp_map_set_reference_order(sageicp_map *map, int on);
int sageicp_map_reference_order(const sageicp_map *map);
/* copy construction / copy assignment (ros/ros2/OdometryServer.cpp:104 copy-assigns the pipeline) */
sageicp_map *sageicp_map_clone(const sageicp_map *map);
int sageicp_map_clear(sageicp_map *map);                    /* Clear(), VoxelHashMap.hpp:93 */
int sageicp_map_empty(const sageicp_map *map);              /* Empty(), VoxelHashMap.hpp:94 */
uint64_t sageicp_map_size(const sageicp_map *map);          /* points held (== Pointcloud().size()) */
uint64_t sageicp_map_num_voxels(const sageicp_map *map);
/* AddPoints, VoxelHashMap.cpp:162-174 (sequential semantic retention policy, .hpp:45-70) */
int sageicp_map_add_points(sageicp_map *map, const double *xyzl, uint64_t n);
/* RemovePointsFarFromLocation, VoxelHashMap.cpp:176-184 */
int sageicp_map_remove_far(sageicp_map *map, const double origin[3]);
/* Update(points, origin), VoxelHashMap.cpp:144-147 */
int sageicp_map_update(sageicp_map *map, const double *xyzl, uint64_t n, const double origin[3]);
/* Update(points, pose), VoxelHashMap.cpp:149-160 */
int sageicp_map_update_pose(sageicp_map *map, const double *xyzl, uint64_t n,
                            const double pose[7]);
/* The same Update(points, pose) executed on the GPU against the HBM-resident map (stable sort by
 * voxel, one lane per voxel run applying VoxelBlock::AddPoint's policy in arrival order, eviction
 * by first-point distance).  Same result as the host entry: identical voxel blocks, free list and
 * counts.  Afterwards the HBM copy is the authority; host-side entries (AddPoints, Pointcloud,
 * clone ...) download it first.  SAGEICP_ERR_CAPACITY if a voxel index exceeds +-2^20. */
int sageicp_map_update_pose_device(sageicp_map *map, const double *xyzl, uint64_t n,
                                   const double pose[7]);
/* Pointcloud(), VoxelHashMap.cpp:132-142.  Returns the number of points the map holds; writes
 * at most `cap` of them (block-pool order; a map in reference-order mode: the reference's bucket order).  While
 * the HBM copy is the authority (after a device-side update) the points are packed on the device
 * and only they cross PCIe: the map stays resident, the next RegisterFrame uploads nothing.
 * `out_xyzl` is typically a fresh allocation (the reference's Pointcloud() returns a new vector):
 * its pages are populated by SAGEICP_TOUCH_THREADS (environment, default 4, 0: off) parked host
 * threads before the copy, which otherwise spends two thirds of its time in first-touch faults. */
uint64_t sageicp_map_pointcloud(const sageicp_map *map, double *out_xyzl, uint64_t cap);
/* 1 while the HBM copy of the map is the authority (device-side updates; Pointcloud() and
 * RegisterFrame keep it so), 0 while the host copy is (AddPoints / Update on the host, Clear). */
int sageicp_map_resident(const sageicp_map *map);
/* Point slots (32 B each) the map's voxel storage occupies, free regions included — the footprint of
 * the point array in HBM and on the host.  Voxels live in size-classed regions (4 / 8 / 16 points,
 * then max_points_per_voxel): a voxel starts in the smallest and moves up when it fills, so a map
 * of sparsely filled voxels does not pay max_points_per_voxel slots for each.  SAGEICP_SIZE_CLASSES=0
 * in the environment when the map is created gives every voxel a full-size region instead. */
uint64_t sageicp_map_point_slots(const sageicp_map *map);
/* Two read-only entries for tests (host-side words only, no device call; additions, the ABI version stays).
 * sageicp_voxel_hash: the hash the slot table is keyed by (home slot = hash & (capacity - 1)).
 * sageicp_map_table_stats: out[0] the capacity of the slot table of whichever copy is the authority, out[1] its used
 * slots (live + tombstoned: the device-side update leaves tombstones, the host table never does), out[2] its live voxels. */
uint32_t sageicp_voxel_hash(int32_t x, int32_t y, int32_t z);
int sageicp_map_table_stats(const sageicp_map *map, uint64_t out[3]);
/* Push pending host-side changes to the HBM mirror now (otherwise done lazily by the next
 * search).  Lets a caller keep the refresh out of a timed region. */
int sageicp_map_sync(const sageicp_map *map);

/* ---- search: VoxelHashMap::GetCorrespondences (core/VoxelHashMap.cpp:48-130) ------------ */
/* src_out / tgt_out: capacity n*4 doubles each; pairs are emitted in query order.
 * query_idx_out (optional, capacity n): index of the query behind each pair. */
int sageicp_get_correspondences(const sageicp_map *map, const double *q_xyzl, uint64_t n,
                                double max_correspondence_distance, double sem_th,
                                double *src_out, double *tgt_out, uint64_t *n_out,
                                int64_t *query_idx_out);

/* ---- Gauss-Newton step: AlignClouds (core/Registration.cpp:59-94) ----------------------- */
/* JTJ_out (36, row-major) and JTr_out (6) are optional.  device: HIP device ordinal. */
int sageicp_align_clouds(const double *src_xyzl, const double *tgt_xyzl, uint64_t n, double kernel,
                         double pose_out[7], double *JTJ_out, double *JTr_out, int device);

/* ---- TransformPoints (core/Registration.hpp:32, Registration.cpp:103-111) ---------------- */
int sageicp_transform_points(const double pose[7], double *xyzl, uint64_t n, int device);

/* ---- RegisterFrame (core/Registration.hpp:34-39, Registration.cpp:113-141) --------------- */
int sageicp_register_frame(const sageicp_map *map, const double *frame_xyzl, uint64_t n,
                           const double initial_guess[7], double max_correspondence_distance,
                           double kernel, double sem_th, double pose_out[7],
                           sageicp_stats *stats /* optional */);

/* The same call on a scan already resident in HBM (what bench.py times), optionally sharded
 * over the ranks of `comm` (NULL: single GPU).  Each rank passes ITS contiguous block of the
 * frame; the map is replicated; the 17 Gauss-Newton sums are all-reduced over RCCL/xGMI every
 * iteration, so every rank returns the same pose. */
sageicp_frame *sageicp_frame_upload(const sageicp_map *map, const double *frame_xyzl, uint64_t n);
void sageicp_frame_destroy(sageicp_frame *frame);
int sageicp_register_frame_resident(const sageicp_map *map, const sageicp_frame *frame,
                                    const double initial_guess[7],
                                    double max_correspondence_distance, double kernel,
                                    double sem_th, sageicp_comm *comm /* optional */,
                                    double pose_out[7], sageicp_stats *stats /* optional */);

/* Which form of the loop the calls of a map handle take, and why.  A frame that fits the machine's LDS runs its whole loop
 * in ONE launch (Registration.cpp:127-138 without a kernel boundary); that launch needs every workgroup resident at once,
 * and when a wait inside it times out (another tenant on the GPU, a driver that places fewer workgroups) the frame is
 * registered through the launch-per-iteration form instead, the handle stays away from the one-launch form for
 * `cooldown_calls` calls and plans `derate_workgroups` fewer workgroups from then on.  The first such event of a process
 * also writes one line to stderr.  Poses are the same to the bit in either form. */
#define SAGEICP_LOOP_FALLBACK_NONE 0
#define SAGEICP_LOOP_FALLBACK_TIMEOUT 1          /* a wait inside the one launch timed out: the grid was not resident as a whole */
#define SAGEICP_LOOP_FALLBACK_COOLDOWN 2         /* the call fell into the cool-down after such a time-out */
#define SAGEICP_LOOP_FALLBACK_DOES_NOT_FIT 3     /* the frame needs more LDS than the machine has (~170k points), or the form is
                                                  * switched off (SAGEICP_LOOP=0), or the call runs under an RCCL communicator */
#define SAGEICP_LOOP_FALLBACK_PEER 4             /* multi-GPU: another rank's one-launch loop timed out; every rank left the same
                                                  * exchange with it and registered the frame again, in step */
typedef struct sageicp_loop_status {
    uint64_t calls_single_launch;       /* registrations of this handle that ran in one launch */
    uint64_t calls_per_iteration;       /* ... through the launch-per-iteration form */
    uint64_t calls_chained;             /* ... of those, with the launches chained: no k_fin between them, the solving wave of the
                                         * one-launch form resident beside them (frames beyond the LDS on one GPU) */
    uint32_t timeouts;                  /* launches that gave up (each cost its time-out, 50 ms by default, before the fall-back) */
    uint32_t cooldown_calls;            /* calls that will still stay away from the one-launch form */
    uint32_t derate_workgroups;         /* workgroups taken off every later plan of this handle (32 per time-out, at most 512) */
    int32_t last_fallback;              /* SAGEICP_LOOP_FALLBACK_*: why the LAST call did not run in one launch (NONE: it did) */
} sageicp_loop_status;
int sageicp_map_loop_status(const sageicp_map *map, sageicp_loop_status *out);

/* ---- query sharding across GPUs (one process per GPU, RCCL over xGMI) -------------------- */
#define SAGEICP_UNIQUE_ID_BYTES 128
int sageicp_comm_unique_id(uint8_t id_out[SAGEICP_UNIQUE_ID_BYTES]);   /* rank 0, then broadcast */
sageicp_comm *sageicp_comm_create(const uint8_t id[SAGEICP_UNIQUE_ID_BYTES], int rank, int nranks,
                                  int device);
void sageicp_comm_destroy(sageicp_comm *comm);

/* Direct exchange of the 20 Gauss-Newton sums between the GPUs of one node, without a collective
 * launch: every rank exports a small block of fine-grained device memory through HIP IPC, maps its
 * peers' blocks, and the workgroup that finishes an iteration stores its sums into every block
 * over xGMI, waits for the others' and solves (replaces ncclAllReduce + a second launch; <= 8
 * ranks).  Usage: export on every rank, all-gather the handles (rank order), connect.  A
 * communicator made by sageicp_comm_create_local() has no RCCL side and only works connected. */
#define SAGEICP_P2P_HANDLE_BYTES 64
sageicp_comm *sageicp_comm_create_local(int rank, int nranks, int device);
int sageicp_comm_p2p_export(sageicp_comm *comm, uint8_t handle_out[SAGEICP_P2P_HANDLE_BYTES]);
int sageicp_comm_p2p_connect(sageicp_comm *comm, const uint8_t *handles /* nranks x 64 B */);
int sageicp_comm_p2p_enable(sageicp_comm *comm, int on);   /* fall back to RCCL with on = 0 */
int sageicp_comm_p2p_enabled(const sageicp_comm *comm);
/* What a communicator is made of, for logs and the bench line: the ranks as given at creation,
 * the ranks RCCL itself reports (ncclCommCount / ncclCommUserRank; -1 without an RCCL side), and the
 * state of the direct exchange. */
typedef struct sageicp_comm_info {
    int32_t rank, nranks, device;
    int32_t has_rccl;        /* 1: created by sageicp_comm_create (an ncclComm_t exists) */
    int32_t rccl_ranks;      /* ncclCommCount, -1: no RCCL side */
    int32_t rccl_rank;       /* ncclCommUserRank, -1: no RCCL side */
    int32_t p2p_connected;   /* every peer's exchange block is mapped */
    int32_t p2p_enabled;     /* the next registration uses the direct exchange */
    int32_t p2p_poisoned;    /* an exchange timed out: the blocks must not be used again */
    int32_t reserved[7];
} sageicp_comm_info;
int sageicp_comm_describe(const sageicp_comm *comm, sageicp_comm_info *out);

/* ---- Preprocess / VoxelDownsample (core/Preprocessing.hpp:33-45) on the device ------------------
 * sageicp_preprocess: core/Preprocessing.cpp:173-187 (dynamic_vehicle_filter == false): keep points
 * with min_range < |p| < max_range, zero the label beyond label_max_range; order preserved.
 * sageicp_voxel_downsample: core/Preprocessing.cpp:44-84: per label group g, the first point that
 * falls into a voxel of size group_voxel_size[g] * vox_scale is kept; points whose label is in no
 * group are dropped.  Output order: see sageicp_set_downsample_order (default: the reference's).
 * out: capacity n*4 doubles.  At most 8 groups; voxel indices must fit +-2^19.  Every group_voxel_size[g] * vox_scale
 * must be finite and above 0, else SAGEICP_ERR_INVALID (sageicp_pipeline_create asks the same of its sizes). */
/* Emission order of sageicp_voxel_downsample and of the pipeline's two down-sampling levels:
 * 1 (default) = the reference's — the bucket order of the tsl::robin_map v1.0.1 its VoxelDownsample
 * iterates (Preprocessing.cpp:76-82), replayed on the host from the survivors' voxel keys, so that
 * the registered cloud and the map get exactly the points the reference's would; 0 = group by group
 * in input order (no host step, ~1 ms less per 120k-pt frame; the poses of a free-running stream
 * then differ from the reference's by centimetres at unchanged accuracy). */
void sageicp_set_downsample_order(int reference_order);
/* The replay itself (host code, no device needed): the iteration order of a tsl::robin_map v1.0.1
 * (core/Preprocessing.cpp:50,76-82: default-constructed, the reference's 20-bit VoxelHash) after the
 * n distinct voxels vox_xyz[3*i..] were inserted in this order; order_out[j] = insertion index of the
 * j-th entry met by the map's iterator.
 * Limits: n < 2^27; SAGEICP_ERR_CAPACITY when an insertion's probe distance reaches 128 — beyond its
 * DIST_FROM_IDEAL_BUCKET_LIMIT tsl::robin_map forces a growth the replay does not model (with the
 * reference's 20-bit hash: at the latest from ~2^19 voxels of one label group; street scenes stay
 * below 40).  Inside sageicp_voxel_downsample / the pipeline such a group is emitted in arrival
 * order and a warning goes to stderr once. */
int sageicp_robin_iteration_order(const int32_t *vox_xyz, uint64_t n, uint32_t *order_out);
/* The far-voxel sweep of VoxelHashMap::RemovePointsFarFromLocation (core/VoxelHashMap.cpp:176-184: erase WHILE iterating the
 * robin_map) on a table filled with the n distinct voxels in arrival order; far[i] != 0: voxel i is out of range.  listed = 0:
 * the sweep as written (every bucket looked at); 1: the form a map whose points live in HBM uses (only the far voxels are
 * known to the host) — the two must agree.  erased_out (capacity n): the voxels erased, in the order of their erasure;
 * order_after (capacity n): the iteration order of what is left. */
int sageicp_robin_sweep(const int32_t *vox_xyz, uint64_t n, const uint8_t *far, int listed, uint32_t *erased_out,
                        uint64_t *n_erased, uint32_t *order_after, uint64_t *n_after);
int sageicp_preprocess(const double *frame_xyzl, uint64_t n, double max_range, double min_range,
                       double label_max_range, double *out_xyzl, uint64_t *n_out, int device);
int sageicp_voxel_downsample(const double *frame_xyzl, uint64_t n, int n_groups,
                             const int *group_label_counts, const int *group_labels,
                             const double *group_voxel_size, double vox_scale, double *out_xyzl,
                             uint64_t *n_out, int device);

/* Preprocess() with dynamic_vehicle_filter == true: core/Preprocessing.cpp:95-172, on the device (dyn_filter.hip).
 * The crop is the filter-off branch's.  A kept point whose label (static_cast<uint32_t>, after zeroing beyond
 * label_max_range) is in dynamic_labels is a vehicle point; the vehicle points are clustered like PCL's
 * EuclideanClusterExtraction (fp32 copies, connected under squared distance < 0.25f, at least 5 points) and a
 * cluster is kept iff its points have more than static_cast<int>(dy_th * size) neighbours within 0.5 m whose label
 * is in landmark_labels.  out (capacity n*4 doubles): the other kept points in frame order, then the kept clusters
 * in PCL's order (sageicp_cluster_emission_order), each in frame order.  Without vehicle points the result is
 * sageicp_preprocess's.  A non-finite label of a kept point refuses the call (SAGEICP_ERR_INVALID).
 * info (optional): what the filter saw.  Assumptions about PCL / FLANN: DESIGN.md, D7. */
typedef struct sageicp_dynfilter_info {
    uint64_t vehicle_points;    /* kept points with a dynamic label */
    uint64_t landmark_points;   /* kept points with a landmark label */
    uint64_t clusters;          /* connected components of >= 5 vehicle points (PCL's clusters) */
    uint64_t clusters_kept;     /* ... that passed the static test (parked vehicles) */
    uint64_t points_removed;    /* vehicle points dropped: moving clusters and components of < 5 points */
    double us_wall;             /* host wall time of the filter, both host round trips included */
    double us_host;             /* of which the host step: waiting for the cluster table, the order replay, the test */
    double us_device;           /* device time of the filter's launches (HIP events; 0 unless sageicp_set_profiling) */
} sageicp_dynfilter_info;
int sageicp_preprocess_dynamic(const double *frame_xyzl, uint64_t n, double max_range, double min_range,
                               double label_max_range, double dy_th, const int *dynamic_labels, int n_dynamic,
                               const int *landmark_labels, int n_landmark, double *out_xyzl, uint64_t *n_out,
                               sageicp_dynfilter_info *info /* optional */, int device);
/* The cluster order replay itself (host code, no device needed): PCL finds the clusters in order of their smallest
 * index, then sorts them with std::sort(rbegin, rend, by size) — largest first, not stable beyond 16 clusters.
 * sizes[k]: size of the k-th cluster found; order_out[j] = k of the j-th cluster emitted (libstdc++'s std::sort). */
int sageicp_cluster_emission_order(const uint32_t *sizes, uint64_t n, uint32_t *order_out);

/* core/Deskew.cpp:36-50 DeSkewScan: out may equal frame_xyzl.  delta = (start.inverse() * finish).log() is formed once
 * on the host; every point i becomes exp((timestamps[i] - 0.5) * delta) * xyz on the device (deskew.hip), with the
 * exponential and point action the ICP update uses (se3_math.h).  The label and the row order are kept.  Poses are
 * {qx, qy, qz, qw, tx, ty, tz} (Sophus::SE3d::data()).  Refused (SAGEICP_ERR_INVALID, nothing written): a NULL pose,
 * a NULL frame / timestamps / out with n > 0, n > 2^26 - 4, and any pose entry, timestamp or point coordinate or label
 * that is not finite.  n == 0 needs no device. */
int sageicp_deskew_scan(const double *frame_xyzl, const double *timestamps, uint64_t n,
                        const double start_pose[7], const double finish_pose[7],
                        double *out_xyzl, int device);

/* ---- per-frame pipeline counterpart: sage_icp::pipeline::sageICP (pipeline/sageICP.{hpp,cpp}) --
 * Host-side orchestration around the hot path for a stream of scans:
 * range crop + label zeroing (core/Preprocessing.cpp:173-187), two-level semantic voxel
 * down-sampling (core/Preprocessing.cpp:44-84, pipeline/sageICP.cpp:97-101), adaptive threshold
 * (core/Threshold.cpp:29-50), constant-velocity guess (pipeline/sageICP.cpp:110-115), RegisterFrame,
 * map update.  The reference's own pipeline compiles unchanged against the header shims; this
 * entry exists so that streams can be driven through the C ABI (tests, bench).  The dynamic vehicle
 * filter (Preprocessing.cpp:95-172) is off by default and switched on with
 * sageicp_pipeline_set_dynamic_vehicle_filter.  Deskewing (pipeline/sageICP.cpp:36-52, core/Deskew.cpp) is off by
 * default, switched on with sageicp_pipeline_set_deskew and applied by sageicp_pipeline_register_frame_timestamps. */
typedef struct sageicp_pipeline sageicp_pipeline;
typedef struct sageicp_pipeline_config {   /* sageConfig, pipeline/sageICP.hpp:39-65 */
    double voxel_size_map, max_range, min_range, label_max_range, local_map_range;
    int basic_points_per_voxel, critical_points_per_voxel;
    const int *basic_parts_labels;
    int n_basic_parts_labels;
    double min_motion_th, initial_threshold, sem_th;
    int n_groups;                     /* voxel_labels.size() == voxel_size.size() */
    const int *group_label_counts;    /* [n_groups] */
    const int *group_labels;          /* concatenated label lists of the groups */
    const double *group_voxel_size;   /* [n_groups] */
    int device;
    int map_update_on_device;         /* 1: the per-frame map update runs on the GPU
                                       * (sageicp_map_update_pose_device); 0: on the host */
} sageicp_pipeline_config;

sageicp_pipeline *sageicp_pipeline_create(const sageicp_pipeline_config *config);
void sageicp_pipeline_destroy(sageicp_pipeline *p);
/* sageICP::RegisterFrame(frame), pipeline/sageICP.cpp:54-95.  icp_seconds is the span the
 * reference times around the hot path (:79-88); n_source the size of the registered cloud. */
int sageicp_pipeline_register_frame(sageicp_pipeline *p, const double *frame_xyzl, uint64_t n,
                                    double pose_out[7], double *icp_seconds, double *total_seconds,
                                    uint64_t *n_source, sageicp_stats *stats /* optional */);
/* Streams: announce the frame that FOLLOWS the next one registered.  Preprocess() + Voxelize()
 * (pipeline/sageICP.cpp:57-67) read the raw frame only — not the pose, not the map — so
 * sageicp_pipeline_register_frame() runs the announced frame's on a second set of device buffers
 * (own stream, own host thread) under the ICP loop and the map update of the frame it was called
 * for, and the call that later registers the announced frame (same pointer, same n) takes the
 * prepared clouds instead of computing them.  Results are bit-identical with and without; a frame
 * that was announced but not registered next is dropped.  One frame ahead, no queue.
 * Lifetime: a helper thread reads the announced buffer from inside the NEXT
 * sageicp_pipeline_register_frame() call on; it has finished when the register call after that one,
 * sageicp_pipeline_prefetch_cancel() or sageicp_pipeline_destroy() returns — until then the buffer
 * must stay valid and unchanged, also when the announced frame ends up not being registered.
 * A frame is recognised by pointer, size AND a fingerprint of its content taken here (64 rows spread
 * over the frame and the last one: best effort — it tells a buffer refilled with another scan from
 * the scan that was announced, not a buffer edited in a few places; do not edit announced buffers).
 * With deskew on (sageicp_pipeline_set_deskew) a frame's Preprocess() reads the deskewed frame, which depends on the
 * pose of the frame registered before it: nothing can be prepared ahead, and this call is SAGEICP_ERR_INVALID. */
int sageicp_pipeline_prefetch(sageicp_pipeline *p, const double *next_frame_xyzl, uint64_t n);
/* Wait for the helper thread without dropping what it prepared: afterwards nothing reads the
 * announced buffer any more (it may be released or refilled), and the prepared clouds are still
 * used if the announced frame — same pointer, size and content — is registered next. */
int sageicp_pipeline_prefetch_wait(sageicp_pipeline *p);
/* Drop an announcement / a prepared frame and wait for the helper thread: afterwards nothing
 * reads any announced buffer. */
int sageicp_pipeline_prefetch_cancel(sageicp_pipeline *p);
/* sageConfig's dynamic_vehicle_filter, dynamic_vehicle_filter_th, dynamic_vehicle_voxid, dynamic_remove_lankmark
 * (pipeline/sageICP.hpp:39-65; used at pipeline/sageICP.cpp:58-65): with enable != 0 every frame goes through
 * sageicp_preprocess_dynamic's filter with dynamic_labels = the config's label group dynamic_vehicle_voxid before it
 * is down-sampled.  Off by default.  An out-of-range voxid is SAGEICP_ERR_INVALID.  A frame prepared by
 * sageicp_pipeline_prefetch under the old setting is dropped (an announcement is kept and prepared under the new). */
int sageicp_pipeline_set_dynamic_vehicle_filter(sageicp_pipeline *p, int enable, double dy_th,
                                                int dynamic_vehicle_voxid, const int *landmark_labels,
                                                int n_landmark);
/* What the filter did to the last frame registered (all zero when it was off). */
int sageicp_pipeline_dynamic_filter_info(const sageicp_pipeline *p, sageicp_dynfilter_info *info);
/* sageConfig::deskew (pipeline/sageICP.hpp:59).  Off by default.  Drops a prepared or announced frame, and while it is
 * on sageicp_pipeline_prefetch is refused (see there).  The one-argument sageicp_pipeline_register_frame never
 * deskews, whatever the setting. */
int sageicp_pipeline_set_deskew(sageicp_pipeline *p, int enable);
/* sageICP::RegisterFrame(frame, timestamps), pipeline/sageICP.cpp:36-52.  Deskew off: timestamps is not read and the
 * call is sageicp_pipeline_register_frame's, bit for bit.  Deskew on: timestamps (n of them) must be non-NULL and
 * finite — checked on every frame, also before the third pose, so a bad stream fails on its first frame
 * (SAGEICP_ERR_INVALID, no pose pushed; the reference does not check).  With three poses or more the
 * frame is deskewed on the device (sageicp_deskew_scan's kernel) with poses N-2 and N-1 before Preprocess(); with
 * fewer it passes through unchanged.  The reference's callers normalise integer stamps first (ros/ros2/Utils.hpp). */
int sageicp_pipeline_register_frame_timestamps(sageicp_pipeline *p, const double *frame_xyzl,
                                               const double *timestamps, uint64_t n, double pose_out[7],
                                               double *icp_seconds, double *total_seconds, uint64_t *n_source,
                                               sageicp_stats *stats /* optional */);
/* Whether the last frame registered was deskewed, and the delta tangent it used (zeros if not). */
int sageicp_pipeline_deskew_info(const sageicp_pipeline *p, int *applied, double delta_out[6]);

/* ---- frames already in device memory (a segmentation network's tensors) --------------------------
 * A raw frame in the caller's device memory, read in place by the ingest kernel (ingest.hip), which writes the
 * library's double[n][4] rows on the device: every value converted with a plain (double) cast (round to nearest, as
 * numpy's astype(float64) or torch's .double()), nothing else — no mask, no label table.  Non-finite values pass
 * through and meet the same checks as host input (the whole call refused, SAGEICP_ERR_INVALID).
 *   xyz    row i starts at xyz + i * xyz_stride bytes; x, y, z are its first three elements (FLOAT32 or FLOAT64).
 *          xyz_stride: a multiple of the element size, at least 3 elements (4 when the label is column 3).
 *   label  NULL: column 3 of the same rows, of xyz_dtype (label_dtype and label_stride are not read);
 *          else element i at label + i * label_stride bytes, UINT8 / INT32 / INT64, stride a multiple of its size.
 * Every extent must be device memory on the handle's device (checked with hipPointerGetAttributes on its first and
 * last byte, before anything is enqueued): host, pinned or managed memory is refused, not copied.
 * Stream: the work that wrote the buffers is ordered before the ingest through an event on `stream` (a hipStream_t
 * of the handle's device; NULL: the null stream).  Lifetime: the calls are synchronous — once one returns, nothing
 * reads the caller's buffers any more (they may be overwritten or freed).  A process must hold ONE HIP runtime:
 * pointers and streams of another runtime loaded beside this library's mean nothing to it. */
#define SAGEICP_DTYPE_FLOAT32 1
#define SAGEICP_DTYPE_FLOAT64 2
#define SAGEICP_DTYPE_UINT8 3
#define SAGEICP_DTYPE_INT32 4
#define SAGEICP_DTYPE_INT64 5
typedef struct sageicp_device_frame {
    const void *xyz;            /* device memory, n rows */
    uint64_t xyz_stride;        /* bytes between rows */
    int32_t xyz_dtype;          /* SAGEICP_DTYPE_FLOAT32 / _FLOAT64 */
    int32_t label_dtype;        /* SAGEICP_DTYPE_UINT8 / _INT32 / _INT64 (label != NULL only) */
    const void *label;          /* device memory, n labels; NULL: column 3 of the rows */
    uint64_t label_stride;      /* bytes between labels (label != NULL only) */
    uint64_t n;                 /* points (at most 2^26 - 4) */
} sageicp_device_frame;
/* sageicp_pipeline_register_frame of a device frame.  timestamps == NULL: sageicp_pipeline_register_frame, bit for
 * bit against the same values given as host rows.  timestamps != NULL (n fp64, contiguous, device memory):
 * sageicp_pipeline_register_frame_timestamps — with deskew off they are not read; with deskew on they are checked on
 * every frame, and a non-finite one is SAGEICP_ERR_INVALID with no pose pushed.  The frame is never one prepared by
 * sageicp_pipeline_prefetch (which takes host frames only); an announcement is consumed by this call as by the host
 * entries. */
int sageicp_pipeline_register_frame_device(sageicp_pipeline *p, const sageicp_device_frame *frame,
                                           const double *timestamps /* device or NULL */,
                                           void *stream /* hipStream_t; NULL = null stream */, double pose_out[7],
                                           double *icp_seconds, double *total_seconds, uint64_t *n_source,
                                           sageicp_stats *stats /* optional */);
/* sageicp_frame_upload of a device frame: the rows are built on the map's device; the result feeds
 * sageicp_register_frame_resident (sharded too) and is released with sageicp_frame_destroy.  NULL on error. */
sageicp_frame *sageicp_frame_from_device(const sageicp_map *map, const sageicp_device_frame *frame,
                                         void *stream /* hipStream_t; NULL = null stream */);

/* ---- outputs into the caller's device memory (egress.hip): the mirror of sageicp_device_frame ---------------------
 * A destination of `cap` rows in the caller's device memory, written in place by the egress kernels.
 *   xyz    row i at xyz + i * xyz_stride bytes; x, y, z are its first three elements (FLOAT32 or FLOAT64).
 *          xyz_stride: a multiple of the element size, at least 3 elements (4 when the label is column 3).
 *          May be NULL only when cap == 0.
 *   label  NULL: column 3 of the same rows, of xyz_dtype (label_dtype and label_stride are not read);
 *          else element i at label + i * label_stride bytes, UINT8 / INT32 / INT64 / FLOAT32 / FLOAT64, the stride a
 *          positive multiple of its size.
 * Which rows: *n_out is the number of rows available, n; the first min(cap, n) of them are written (as
 * sageicp_map_pointcloud does) and the rest of the destination is not touched.
 * Conversions: float64 coordinates are written bit for bit, float32 ones through a plain (float) cast (round to
 * nearest, as numpy's astype(float32)); a float label is a plain cast; an integer label is static_cast<int64_t>(label)
 * (the reference's cast) and must then fit the label's type — one that does not (259 into UINT8, say) makes the call
 * SAGEICP_ERR_INVALID, and the destination's contents are then unspecified.
 * Checks, before anything is enqueued: the layout above; every extent of `cap` rows must be device memory on the
 * handle's device (hipPointerGetAttributes on its first and last byte): host, pinned or managed memory is refused,
 * not copied.
 * Stream: the caller's earlier work on `stream` (a hipStream_t of the handle's device; NULL: the null stream) is
 * ordered before the write through an event — a caching allocator hands out blocks that earlier kernels on that
 * stream may still be using.  Lifetime: the calls are synchronous — once one returns, the rows are in place and
 * nothing of the library touches the destination any more. */
typedef struct sageicp_device_points {
    void *xyz;                  /* device memory, cap rows */
    uint64_t xyz_stride;        /* bytes between rows */
    int32_t xyz_dtype;          /* SAGEICP_DTYPE_FLOAT32 / _FLOAT64 */
    int32_t label_dtype;        /* SAGEICP_DTYPE_UINT8 / _INT32 / _INT64 / _FLOAT32 / _FLOAT64 (label != NULL only) */
    void *label;                /* device memory, cap labels; NULL: column 3 of the rows */
    uint64_t label_stride;      /* bytes between labels (label != NULL only) */
    uint64_t cap;               /* rows the destination holds */
} sageicp_device_points;
/* The source cloud of the last frame registered (RegisterFrame's `source`, pipeline/sageICP.cpp:94): the n_source rows
 * that were registered, through any entry (host rows, timestamps, device frame; with or without prefetch, deskew or
 * the dynamic filter), as double[n][4] host rows.  out_xyzl may be NULL only when cap == 0 (*n_out then tells n).
 * Order: the pipeline's own — arrival order within each label group by default, a permutation of the reference's
 * `source`; the reference's bucket order under SAGEICP_SOURCE_REFERENCE_ORDER=1.  0 rows before the first frame,
 * after a register call that failed and after sageicp_pipeline_reinitialize.  Valid until the next register call. */
int sageicp_pipeline_source(const sageicp_pipeline *p, double *out_xyzl, uint64_t cap, uint64_t *n_out);
/* the same rows into the caller's device memory */
int sageicp_pipeline_source_device(const sageicp_pipeline *p, const sageicp_device_points *dst,
                                   void *stream /* hipStream_t; NULL = null stream */, uint64_t *n_out);
/* sageicp_map_pointcloud's rows, in its order (the bucket order in reference-order mode), into the caller's device
 * memory; packed on the device straight into the destination while the HBM copy is the authority, staged from the
 * host copy while it is not */
int sageicp_map_pointcloud_device(const sageicp_map *m, const sageicp_device_points *dst,
                                  void *stream /* hipStream_t; NULL = null stream */, uint64_t *n_out);
/* VoxelHashMap::GetCorrespondences (core/VoxelHashMap.cpp:48-130) of a frame in device memory, answered into device memory.
 * Inputs: the frame is read through sageicp_pipeline_register_frame_device's conversion (a plain (double) cast).  With
 * pose != NULL every row is first moved by the point action of sageicp_transform_points, bit for bit, its label kept:
 * the moved rows are the queries (Registration.cpp:123,129).  A pose, coordinate or label that is not finite refuses
 * the whole call (SAGEICP_ERR_INVALID) before anything is written to a destination.
 * Result: *n_out pairs, in query order, exactly sageicp_get_correspondences': pair k has src = the k-th accepted query
 * row (with a pose: the moved row), tgt = that query's semantic nearest neighbour, bit for bit the map's row, and
 * query_idx_out[k] = the query's index in the frame.  A query with no point in its 27 voxels gives no pair; an empty
 * map or n == 0 gives 0 pairs and reads nothing.
 * Capacity: any of src_out, tgt_out, query_idx_out may be NULL (all three: a count-only call); the caps of those given
 * — src_out->cap, tgt_out->cap, idx_cap — must be equal.  The first min(cap, *n_out) pairs are written and nothing
 * beyond them is touched.  Conversions into src_out / tgt_out are sageicp_device_points' own, the refusal of an integer
 * label that does not fit included (the destinations' contents are then unspecified).
 * Checks, before anything is enqueued: the three layouts first (no device is asked); the caps; query_idx_out 8-byte
 * aligned; destinations that overlap EACH OTHER are refused (their extents are compared on the host); then every extent
 * must be device memory of the map's device, and the stream one of it.  A destination MAY alias the frame: the frame is
 * ingested completely into the library's own rows before any destination is written — guaranteed.
 * Stream and lifetime: as for sageicp_device_frame and sageicp_device_points — the caller's earlier work on `stream` is
 * ordered before the call's through an event; the call is synchronous: on return the pairs are in place and nothing
 * reads or writes the caller's memory.
 * Map state: the target rows come from the HBM copy of the map, as a mirror (refreshed like before any search) or as the
 * authority: nothing is downloaded, and sageicp_map_resident, sageicp_map_table_stats and sageicp_map_loop_status answer
 * after the call what they answered before it.  (sageicp_get_correspondences reads the host copy and hands a resident
 * map back to the host.)  A map that spans several devices answers on the first. */
int sageicp_get_correspondences_device(const sageicp_map *map, const sageicp_device_frame *frame,
                                       const double pose[7] /* NULL = identity */,
                                       double max_correspondence_distance, double sem_th,
                                       const sageicp_device_points *src_out /* or NULL */,
                                       const sageicp_device_points *tgt_out /* or NULL */,
                                       int64_t *query_idx_out /* device, or NULL */, uint64_t idx_cap,
                                       void *stream /* hipStream_t; NULL = null stream */, uint64_t *n_out);

/* ---- registration quality (quality.hip) -------------------------------------------------------------------------------
 * How good a pose is, from one fused pass on the device behind the search: what Open3D's registration result calls
 * fitness, inlier_rmse and the information matrix, the Gauss-Newton step still left at the pose, a covariance for
 * nav_msgs/Odometry, and — for a semantic ICP — which classes produced the pairs and how the pairs split by the label
 * rule of core/VoxelHashMap.cpp:88.
 *
 * Inputs: a map, a frame of n rows, an optional pose applied to the rows exactly as sageicp_get_correspondences_device
 * applies its pose, max_correspondence_distance, kernel (k) and sem_th.  The accepted pairs are exactly those of
 * GetCorrespondences for the same arguments: the same search, the same acceptance test, query order.
 * For an accepted pair with moved query s (label ls) and map point q (label lq):
 *     r = s - q,   e = |r|^2,   w = k^2 / (k + e)^2,   J = [ I | -hat(s) ]            (core/Registration.cpp:59-94)
 * Sums over the accepted pairs: n_pairs; sum_r2 = sum e; sum_w = sum w; sum_w_r2 = sum w e; JTJ = sum w J^T J (6x6,
 * row-major); JTr = sum w J^T r; info = sum J^T J, unweighted (Open3D's information matrix).
 * Derived on the host in fp64 from the sums:
 *     fitness = n_pairs / n_queries;   rmse = sqrt(sum_r2 / n_pairs), 0 without pairs;
 *     step = -JTJ^-1 JTr, the Gauss-Newton step still left at this pose, and step_norm its 2-norm;
 *     covariance = s2 JTJ^-1 with s2 = sum_w_r2 / (3 n_pairs - 6), in the tangent the loop composes with,
 *         T <- exp(x) T, x = (upsilon, omega) (Registration.cpp:135);
 *     covariance_pose = G covariance G^T with G = [[I, -hat(t)], [0, I]], t the pose's translation (0 without a pose):
 *         the covariance of the pose's own translation and world-axis rotation (dt = upsilon - hat(t) omega,
 *         dtheta = omega), row-major in the order x, y, z, rot x, rot y, rot z: nav_msgs/Odometry.pose.covariance.
 * covariance_valid = 1 only if n_pairs >= 3 and the Cholesky factorisation of JTJ has six positive pivots, each above
 * 2^-26 of its diagonal entry (a pivot far below is the rounding of a zero: collinear pairs; one at the bound keeps half of
 * fp64's digits — a 30 m scene at UTM coordinates lies below it: register in a local frame for a covariance there);
 * otherwise step, step_norm and the two covariances are zero and the flag is 0.
 * Classes: the class of a query is static_cast<int>(ls); classes 0 .. 255 are counted per class (class_queries: every
 * query; class_pairs, class_sum_r2: the accepted ones), anything else in other_*.  The split of the pairs:
 * pairs_same_label: (int)lq == (int)ls; pairs_unlabelled: not same and (int)(lq * ls) == 0; pairs_cross_label: the rest.
 * valid = 0 for an empty map or n == 0: everything else is zero then, and the call returns SAGEICP_OK.
 * Bits: the results depend on the rows, their order and the arguments, and on nothing else: two calls, the host-rows
 * entry, the device-frame entry on the same float64 rows and the pipeline's evaluation of the same rows agree bit for
 * bit.  Sums are fp64 (no fixed-point range: coordinates of any finite size keep their relative accuracy). */
typedef struct sageicp_quality {
    double fitness, rmse, step_norm;
    double sum_r2, sum_w, sum_w_r2;
    double step[6];
    double JTr[6];
    double JTJ[36];
    double info[36];
    double covariance[36];
    double covariance_pose[36];
    double class_sum_r2[256];
    double other_sum_r2;
    uint64_t n_queries, n_pairs;
    uint64_t pairs_same_label, pairs_unlabelled, pairs_cross_label;
    uint64_t other_queries, other_pairs;
    uint32_t class_queries[256];
    uint32_t class_pairs[256];
    int32_t valid, covariance_valid;
} sageicp_quality;                                                 /* 5464 bytes, no padding */
/* Refused with SAGEICP_ERR_INVALID before any device work: a null map or out; a pose that is not finite; a kernel that is
 * not finite or not above 0; rows that are not finite (the host scan). */
int sageicp_registration_quality(const sageicp_map *map, const double *xyzl, uint64_t n,
                                 const double pose[7] /* NULL = identity */, double max_correspondence_distance,
                                 double kernel, double sem_th, sageicp_quality *out);
/* The same on a frame in device memory: every layout and dtype of sageicp_get_correspondences_device, through the same
 * checks of the caller's memory; non-finite rows are refused by the sort's verdict.  Synchronous.  The map stays where it
 * is: a resident map stays resident.  A map that spans several devices answers on the first. */
int sageicp_registration_quality_device(const sageicp_map *map, const sageicp_device_frame *frame,
                                        const double pose[7] /* NULL = identity */, double max_correspondence_distance,
                                        double kernel, double sem_th, void *stream /* hipStream_t; NULL = null stream */,
                                        sageicp_quality *out);
/* In the pipeline: off by default.  When on, every register call evaluates the report for its source cloud at the NEW
 * pose, with that frame's 3 sigma and sigma / 3, against the map BEFORE Update() inserts the frame — after the
 * registration, outside the icp_s and total_s it reports.  The first frame (empty map) and an empty message give
 * valid = 0; so does a register call that fails, and sageicp_pipeline_reinitialize. */
int sageicp_pipeline_set_quality(sageicp_pipeline *p, int enable);
int sageicp_pipeline_quality(const sageicp_pipeline *p, sageicp_quality *out);

/* ---- a batch of candidate poses scored in one pass; relocalisation (score.hip) ----------------------------------------
 * Moved by k poses, a frame of n rows is k * n independent queries against the same map: one search answers all of them,
 * and one pass forms every candidate's sums.  out[c] holds, bit for bit, the same-named fields of
 * sageicp_registration_quality(map, xyzl, n, poses[c], ...) — fitness, rmse, step_norm, sum_r2, sum_w, sum_w_r2, step,
 * JTr, JTJ, n_queries, n_pairs, the three splits of the pairs, valid —, step_valid is that report's covariance_valid and
 * score, the ranking key, is sum_w.  This holds whatever k is, whatever the other candidates are and in whatever order,
 * and however the batch was cut into chunks.  The class tables, `info` and the covariances are not formed in the batch:
 * ask sageicp_registration_quality at the pose that won.
 * Chunks: the candidates are taken max(1, chunk_rows / n) at a time, chunk_rows from SAGEICP_SCORE_CHUNK_ROWS (default
 * 2^20 rows; about 250 B of device memory per row, which stays reserved on the map handle like its other work buffers);
 * per chunk the sort's verdict on non-finite rows is read once and the results are downloaded once.
 * k == 0: SAGEICP_OK, nothing read or written.  An empty map or n == 0: every out[c] is zero (valid = 0), SAGEICP_OK.
 * Refused with SAGEICP_ERR_INVALID before any device is asked (k > 0): a null map, out or poses; null rows with n > 0;
 * k > 2^20; n > 2^26 - 4; a kernel that is not finite or not above 0; a pose entry that is not finite (the message
 * names the candidate).  The host entry scans its rows; in both entries the sort's verdict refuses rows that are not
 * finite once moved.  On every error nothing has been written to out.
 * The map stays where it is: a resident map stays resident, and sageicp_map_table_stats and sageicp_map_loop_status
 * answer after the call what they answered before it.  A map that spans several devices answers on the first. */
typedef struct sageicp_pose_score {
    double score;                            /* the ranking key: sum_w */
    double fitness, rmse, step_norm;
    double sum_r2, sum_w, sum_w_r2;
    double step[6], JTr[6], JTJ[36];
    uint64_t n_queries, n_pairs, pairs_same_label, pairs_unlabelled, pairs_cross_label;
    int32_t valid, step_valid;
} sageicp_pose_score;                                              /* 488 bytes, doubles first, no padding */
int sageicp_score_poses(const sageicp_map *map, const double *xyzl, uint64_t n,
                        const double *poses /* [k][7] */, uint64_t k,
                        double max_correspondence_distance, double kernel, double sem_th,
                        sageicp_pose_score *out /* [k] */);
/* The same on a frame in device memory: the layout and caller-memory checks of sageicp_registration_quality_device.
 * Synchronous. */
int sageicp_score_poses_device(const sageicp_map *map, const sageicp_device_frame *frame,
                               const double *poses /* host, [k][7] */, uint64_t k,
                               double max_correspondence_distance, double kernel, double sem_th,
                               void *stream /* hipStream_t; NULL = null stream */, sageicp_pose_score *out);

/* Relocalisation: a grid of candidates around a prior, scored in one batch, the best few refined by RegisterFrame.
 * Candidates (host code, no device needed).  Per axis, m is the largest integer >= 0 with m * step <= extent in fp64,
 * and 0 when step <= 0 or extent < step; the indices run from -m to +m.  Candidate (a, i, j, l) is the sensor turned in
 * place about the vertical through its own position, then shifted along the world axes:
 *     q = q_z(a * yaw_step) (x) q_prior  (Hamilton product, not renormalised; q_z(th) = (0, 0, sin(th / 2), cos(th / 2)));
 *     t = t_prior + (i * xy_step, j * xy_step, l * z_step);
 * an index of 0 leaves the prior's own bits.  Order: yaw outermost, then x, then y, z innermost, each ascending.
 * k_out always tells K; the first min(cap, K) poses are written (poses_out may be NULL with cap == 0).
 * SAGEICP_ERR_INVALID: K > 2^20, a prior or a parameter that is not finite, refine_top > 16.
 * sageicp_relocalize is a composition of public entries: (1) the candidates; (2) sageicp_score_poses; (3) the ranking by
 * score, descending, ties to the lower index; (4) for the first min(refine_top, K) of them RegisterFrame from the
 * candidate — the bits of sageicp_register_frame(map, xyzl, n, candidate, max_correspondence_distance, kernel, sem_th)
 * — and sageicp_registration_quality at its result; the winner is the largest sum_w, ties to the better rank; (5) with
 * refine_top == 0 the best candidate itself is returned.  quality_out is the full report at pose_out.  The frame is
 * uploaded (ingested) once and stays on the device through all steps.  An empty map or n == 0 returns the prior,
 * valid = 0 and refined = 0.  The ranking key cannot tell two poses apart that explain the scan equally well (the two
 * directions of a symmetric street): keep the extents as small as the prior allows. */
typedef struct sageicp_relocalize_params {
    double xy_extent, xy_step, z_extent, z_step;   /* metres, world axes */
    double yaw_extent, yaw_step;                   /* radians about world z */
    uint32_t refine_top, reserved;                 /* 0 .. 16 */
    double max_correspondence_distance, kernel, sem_th;
} sageicp_relocalize_params;                                       /* 80 bytes */
typedef struct sageicp_relocalize_info {
    uint64_t candidates, best_candidate;   /* best_candidate: index of the candidate the returned pose came from */
    double best_candidate_score;           /* its score before refinement */
    uint32_t refined, winner_rank;         /* registrations run; rank (0 = best score) of the winner among them */
    int32_t iterations, converged;         /* of the winner's registration (0, 0 with refine_top == 0) */
    double us_score, us_refine, us_wall;
} sageicp_relocalize_info;                                         /* 64 bytes */
int sageicp_relocalize_candidates(const double prior[7], const sageicp_relocalize_params *params,
                                  double *poses_out /* [cap][7] */, uint64_t cap, uint64_t *k_out);
int sageicp_relocalize(const sageicp_map *map, const double *xyzl, uint64_t n, const double prior[7],
                       const sageicp_relocalize_params *params, double pose_out[7],
                       sageicp_quality *quality_out /* optional */, sageicp_relocalize_info *info /* optional */);
int sageicp_relocalize_device(const sageicp_map *map, const sageicp_device_frame *frame, const double prior[7],
                              const sageicp_relocalize_params *params, void *stream, double pose_out[7],
                              sageicp_quality *quality_out, sageicp_relocalize_info *info);

int sageicp_pipeline_reinitialize(sageicp_pipeline *p);          /* pipeline/sageICP.hpp:94-99 */
uint64_t sageicp_pipeline_num_poses(const sageicp_pipeline *p);  /* poses().size() */
int sageicp_pipeline_pose(const sageicp_pipeline *p, uint64_t index, double pose_out[7]);
const sageicp_map *sageicp_pipeline_local_map(const sageicp_pipeline *p);   /* LocalMap() */

/* ---- key-frame selection by occupancy overlap (keyframe.hip) ---------------------------------------------------------
 * The odometry node's key-frame choice (ros/ros2/OdometryServer.cpp:222-243, ros/ros2/Utils.hpp:221-260), run on the
 * device.  A grid is a bird's-eye occupancy of H rows (y) by W columns (x), cell (y, x) at byte y * W + x of a grid
 * written out: a point is skipped unless lo <= v <= hi on all three axes; it sets the cell
 *     occ_x = (int)((x + bounds[0][1]) / ((bounds[0][1] - bounds[0][0]) / W)),
 *     occ_y = (int)((y + bounds[1][1]) / ((bounds[1][1] - bounds[1][0]) / H))
 * when 0 <= occ_x < W and 0 <= occ_y < H — the UPPER bound is the offset, as in the reference, and the cast truncates
 * toward zero (fp64, a true division; the range is tested on the double before the cast).
 * Refused (SAGEICP_ERR_INVALID): bounds that are not finite or lo >= hi on an axis, occ_h or occ_w outside [1, 4096],
 * an overlap_th that is not finite. */
typedef struct sageicp_occupancy_params {
    double bounds[3][2];        /* (lo, hi) of x, y, z; key_frame_bounds of the launch files */
    int32_t occ_h, occ_w;       /* key_frame_occ_size: rows (y), columns (x) */
    double overlap_th;          /* key_frame_overlap: a frame whose overlap is below becomes the key frame */
} sageicp_occupancy_params;
typedef struct sageicp_key_frame_info {
    int32_t enabled;            /* selection is on */
    int32_t is_key_frame;       /* the last frame registered became the key frame */
    double overlap;             /* |key & cur| / |key| of the last frame; NaN on a first key frame or when |key| = 0 */
    uint64_t key_frame_index;   /* the key frame's index in the poses (valid while key_frames > 0) */
    uint64_t key_frames;        /* key frames taken since selection was switched on or reset */
    uint64_t key_occupied;      /* |key|: occupied cells of the key grid the last frame was compared with (0 on a first) */
    uint64_t intersect;         /* |key & cur| of that comparison */
    double key_pose[7];         /* the key frame's pose (identity while there is none) */
} sageicp_key_frame_info;
/* Key-frame selection for every frame the pipeline registers (host rows, timestamps, device frames, prefetched frames),
 * after its pose is pushed and outside the times the register calls report.  The input is the RAW frame as handed in
 * (before deskew, the dynamic filter and the crop); with no key frame yet the frame becomes the key frame, otherwise
 * it is drawn under key_pose^-1 * pose and becomes the key frame when its overlap with the key grid is below
 * overlap_th (the stored grid is the frame's own, untransformed).  While it is on, a frame with a coordinate that is
 * not finite is refused whole (no pose pushed); a register call that fails changes nothing of the selection.  Off by
 * default; off, nothing of it runs.  Switching it on (or setting new params) starts from "no key frame"; params may
 * be NULL when enable == 0.  sageicp_pipeline_reinitialize keeps the state (the node's ReinitService does); _reset
 * clears it. */
int sageicp_pipeline_set_key_frames(sageicp_pipeline *p, int enable, const sageicp_occupancy_params *params);
int sageicp_pipeline_key_frame_reset(sageicp_pipeline *p);
int sageicp_pipeline_key_frame_info(const sageicp_pipeline *p, sageicp_key_frame_info *info);
/* the key grid as occ_h * occ_w bytes (0 / 1; zeros while there is no key frame); cap: bytes at out, at least
 * occ_h * occ_w.  SAGEICP_ERR_INVALID while selection is off. */
int sageicp_pipeline_key_frame_grid(const sageicp_pipeline *p, uint8_t *out, uint64_t cap);
/* the same bytes into the caller's device memory, with sageicp_device_points' checks and stream rules (the extent must
 * be device memory of the pipeline's device; ordered behind the work on `stream`; synchronous) */
int sageicp_pipeline_key_frame_grid_device(const sageicp_pipeline *p, uint8_t *out, uint64_t cap,
                                           void *stream /* hipStream_t; NULL = null stream */);
/* The grid of n host rows, moved by `pose` first (NULL: identity; the point action of sageicp_transform_points, bit for
 * bit), into occ_h * occ_w host bytes; params->overlap_th is checked but not used.  A coordinate or a pose that is not
 * finite refuses the call. */
int sageicp_occupancy_grid(const double *xyzl, uint64_t n, const double pose[7] /* NULL = identity */,
                           const sageicp_occupancy_params *params, uint8_t *grid_out, int device);
/* the same of a frame in device memory (sageicp_device_frame, read through the same conversion as
 * sageicp_pipeline_register_frame_device, on the device its memory lives on and behind the work on `stream`); the grid
 * goes to host memory.  Synchronous. */
int sageicp_occupancy_grid_device(const sageicp_device_frame *frame, const double pose[7] /* NULL = identity */,
                                  const sageicp_occupancy_params *params, uint8_t *grid_out,
                                  void *stream /* hipStream_t; NULL = null stream */);

/* ---- sensor_msgs/PointCloud2 payloads (msg.hip): the odometry node's two message conversions ---------------------------
 * ros/ros2/Utils.hpp:55-198 on the device (additions only, the ABI version stays): PointCloud2ToEigen + GetTimestamps
 * at the input (OdometryServer.cpp:160-167), EigenToPointCloud2 at the two outputs (:214, :219).  Little-endian only.
 *
 * Input.  An incoming message's `data` as n = height * width records of point_step bytes (the reference's iterators
 * step by point_step and ignore row_step; so does this).  x, y, z are FLOAT32, the label UINT8 or FLOAT32, the stamp
 * uint32 or float64, each at any byte offset; neither `data` nor point_step need be a multiple of 4.  Every value
 * becomes a double through a plain cast.  uint32 stamps follow NormalizeTimestamps (Utils.hpp:68-77): with their maximum
 * below 1 (all zero) they stay as cast, otherwise each is (double)t / (double)max, an fp64 division; float64 stamps
 * pass through unchanged. */
typedef struct sageicp_msg_layout {      /* an incoming PointCloud2's fields, as PointCloud2ToEigen / GetTimestamps read them */
    uint32_t point_step;                 /* bytes between points; every field used ends within it; at most 1024 */
    uint32_t x_offset, y_offset, z_offset;   /* FLOAT32 */
    uint32_t label_offset;  int32_t label_dtype;   /* SAGEICP_DTYPE_UINT8 or _FLOAT32 */
    int32_t  time_kind;                  /* 0 none; 1 uint32, normalised by its maximum; 2 float64 as is */
    uint32_t time_offset;
} sageicp_msg_layout;
/* the node's color_list (std::map<int, int>): n (key, value) pairs; a later pair with the same key wins */
typedef struct sageicp_msg_colors { const int32_t *keys, *values; uint32_t n; } sageicp_msg_colors;
/* sageicp_pipeline_register_frame of a message in host memory: the n * point_step raw bytes cross PCIe (not 32-byte
 * rows) and are unpacked into the pipeline's buffers on its stream.
 * From the point where the rows are on the device the frame is treated as sageicp_pipeline_register_frame_device treats
 * a device frame — key frames on the raw rows, the dynamic filter, an announcement of sageicp_pipeline_prefetch consumed,
 * the non-finite checks — and the pose is bit for bit what the same values give as host rows.
 * Deskew off: the time field is never read, whatever time_kind says (OdometryServer.cpp:161-164).
 * Deskew on and time_kind == 0: SAGEICP_ERR_INVALID, no pose pushed.
 * Deskew on with stamps: they are read and checked on every frame, as sageicp_pipeline_register_frame_timestamps does
 * (a float64 stamp that is not finite: SAGEICP_ERR_INVALID, no pose pushed).
 * n == 0 is a valid empty frame and reads nothing (the reference's max_element of no stamps is undefined).
 * Refused before anything is enqueued and without needing a device (SAGEICP_ERR_INVALID): a NULL layout; point_step 0
 * or above 1024; a field that ends beyond point_step; a label_dtype or time_kind other than the above;
 * data_bytes < n * point_step (the reference would read out of bounds); n > 2^26 - 4; NULL data with n > 0. */
int sageicp_pipeline_register_frame_msg(sageicp_pipeline *p, const void *data, uint64_t data_bytes, uint64_t n,
                                        const sageicp_msg_layout *layout, double pose_out[7], double *icp_seconds,
                                        double *total_seconds, uint64_t *n_source, sageicp_stats *stats /* optional */);
/* the same of a message whose data is in the caller's device memory, with sageicp_device_frame's checks and stream
 * rules: the first and the last byte of the n * point_step extent must be device memory of the pipeline's device (host,
 * pinned and managed memory are refused, not copied); the read is ordered behind the work on `stream`; synchronous. */
int sageicp_pipeline_register_frame_msg_device(sageicp_pipeline *p, const void *data, uint64_t data_bytes, uint64_t n,
                                               const sageicp_msg_layout *layout,
                                               void *stream /* hipStream_t; NULL = null stream */, double pose_out[7],
                                               double *icp_seconds, double *total_seconds, uint64_t *n_source,
                                               sageicp_stats *stats /* optional */);
/* Output.  The record CreatePointCloud2Msg + FillPointCloud2XYZlRGB write (Utils.hpp:104-145), point_step 21:
 *   bytes 0-11  x, y, z as (float) casts          byte 12  the label as uint8
 *   bytes 13-16 rgb: the colour of (int)label, the table's int converted to uint32_t
 *   bytes 17-20 zero (the bytes data.resize leaves)
 * Label rule: trunc(label) must lie in [0, 255] (-0.5 gives 0; 256 does not fit: where static_cast<uint8_t> is defined).
 * Colour rule: the table must hold a colour for (int)label (the reference's map::at throws where it does not); keys
 * outside 0..255 can never match and are ignored.  A row that breaks either rule makes the call SAGEICP_ERR_INVALID, and
 * the destination's contents are then unspecified. */
#define SAGEICP_MSG_POINT_STEP 21
#define SAGEICP_MSG_X_OFFSET 0
#define SAGEICP_MSG_Y_OFFSET 4
#define SAGEICP_MSG_Z_OFFSET 8
#define SAGEICP_MSG_LABEL_OFFSET 12
#define SAGEICP_MSG_RGB_OFFSET 13
/* sensor_msgs/PointField datatype codes */
#define SAGEICP_MSG_FIELD_UINT8 2
#define SAGEICP_MSG_FIELD_UINT32 6
#define SAGEICP_MSG_FIELD_FLOAT32 7
#define SAGEICP_MSG_FIELD_FLOAT64 8
typedef struct sageicp_msg_field { char name[8]; uint32_t offset; int32_t datatype; uint32_t count; } sageicp_msg_field;
/* the outgoing record's field table (x, y, z, label, rgb), for msg.fields: returns the number of fields, writes the
 * first min(cap, that) of them.  No device needed. */
uint32_t sageicp_msg_output_fields(sageicp_msg_field *out, uint32_t cap);
/* sageicp_pipeline_source's rows, in its order, as 21-byte records in host memory: *n_out is the number of rows there
 * are, the first min(cap_points, n) are written (min(cap_points, n) * 21 bytes, no byte beyond them).  out may be NULL
 * only when cap_points == 0.  colors: NULL or n == 0 is an empty table; n > 0 with a NULL array is refused. */
int sageicp_pipeline_source_msg(const sageicp_pipeline *p, const sageicp_msg_colors *colors, void *out,
                                uint64_t cap_points, uint64_t *n_out);
/* the same into the caller's device memory (any alignment), with sageicp_device_points' checks and stream rules: the
 * extent of cap_points * 21 bytes must be device memory of the handle's device; ordered behind the work on `stream`;
 * synchronous */
int sageicp_pipeline_source_msg_device(const sageicp_pipeline *p, const sageicp_msg_colors *colors, void *out,
                                       uint64_t cap_points, void *stream /* hipStream_t; NULL = null stream */,
                                       uint64_t *n_out);
/* sageicp_map_pointcloud's rows, in its order (the bucket order in reference-order mode), as 21-byte records: packed on
 * the device from the HBM copy while it is the authority, staged from the host copy while it is not (as
 * sageicp_map_pointcloud_device); either way the records are written on the device */
int sageicp_map_pointcloud_msg(const sageicp_map *map, const sageicp_msg_colors *colors, void *out, uint64_t cap_points,
                               uint64_t *n_out);
int sageicp_map_pointcloud_msg_device(const sageicp_map *map, const sageicp_msg_colors *colors, void *out,
                                      uint64_t cap_points, void *stream /* hipStream_t; NULL = null stream */,
                                      uint64_t *n_out);

/* ---- the archive of a map: what the local map evicts, and the session's map --------------------------
 * A per-handle, append-only log of the voxels RemovePointsFarFromLocation evicts; off by default, and with it off no
 * call does anything it did not do before.  While it is on, every voxel that sageicp_map_remove_far, sageicp_map_update,
 * sageicp_map_update_pose, sageicp_map_update_pose_device or the pipeline's per-frame update evicts is appended before
 * its block is freed — on the device for an update that runs there (new kernels between the search for the far voxels
 * and their eviction, no atomic deciding a position, no added host synchronisation), on the host otherwise.
 * Order: calls in the order they were made; within a call the voxels in the order of their eviction (ascending block
 * index; in reference-order mode the order the erase-while-iterating sweep erases them); within a voxel its rows in
 * their stored order, bit for bit.  A refused update (non-finite input, a voxel index beyond +-2^20, storage overflow)
 * leaves what the archive holds unchanged and takes no serial (where its rows are kept may change: a device-side update
 * first moves rows that host-side evictions left on the host behind the device part and reserves room, which can
 * re-allocate the device buffers and then waits for the stream; an update that does neither adds no synchronisation).
 * Limit: max_rows (0: none).  A voxel is archived only while all its rows still fit; the first that does not makes the
 * archive `full` until sageicp_map_archive_clear, and evictions are only counted from then on (dropped_rows /
 * dropped_voxels): a limited archive is the longest prefix of whole voxels of the unlimited one.
 * Lifetime: sageicp_map_clear and sageicp_pipeline_reinitialize leave the archive alone (it belongs to the session, not
 * to the window); sageicp_map_archive_clear empties it, releases its device memory, resets full, the dropped counts and
 * the serial, and keeps the setting; sageicp_map_clone copies setting and contents; of a multi-device map only the first
 * copy archives.  Environment (for callers behind the header shim): SAGEICP_MAP_ARCHIVE=1 switches it on for every map
 * the process creates, SAGEICP_MAP_ARCHIVE_MAX_ROWS sets the limit (a 64-bit decimal count of rows).
 * Exports — `which`: SAGEICP_ARCHIVE_ALL the log as recorded (a voxel the sensor came back to and left again appears once
 * per generation); SAGEICP_ARCHIVE_LATEST record i iff no later record has its key and the live map holds no voxel with
 * that key, in log order; SAGEICP_SESSION the LATEST rows followed by sageicp_map_pointcloud's rows in its order: every
 * voxel key the session has seen exactly once, with its most recent content.  `first` skips rows of the selection;
 * *n_out = the rows the selection has; rows [first, first + min(cap, *n_out - first)) are written and nothing beyond
 * them; first > *n_out writes nothing and is SAGEICP_OK.  Exports are synchronous, work whether the archive is on or
 * off, and follow sageicp_map_pointcloud_device's stream and lifetime rules and sageicp_map_pointcloud_msg's colour and
 * label rules.  ALL into host rows needs no device while no row of the archive is in device memory; every other export
 * is device work (SAGEICP_ERR_NO_DEVICE without one) and leaves a resident map resident. */
#define SAGEICP_ARCHIVE_ALL 0
#define SAGEICP_ARCHIVE_LATEST 1
#define SAGEICP_SESSION 2
typedef struct sageicp_archive_info {
    int32_t enabled, full;
    uint64_t rows, voxels, dropped_rows, dropped_voxels, max_rows, updates;
    uint64_t device_rows, host_rows, device_bytes;   /* where the rows are; what the archive holds in device memory */
} sageicp_archive_info;
typedef struct sageicp_archive_voxel {
    int32_t x, y, z;       /* the voxel key */
    uint32_t count;
    uint64_t first_row;    /* index of its first row in the log */
    uint64_t update;       /* serial of the call that evicted it: the eviction-capable calls that succeeded before it
                              while the archive was on, counted since the map was created or the archive cleared (a call
                              that evicts nothing takes one too; calls made while it is off take none, and switching it
                              off and on again goes on counting where it stopped) */
} sageicp_archive_voxel;
int sageicp_map_set_archive(sageicp_map *m, int enable, uint64_t max_rows);   /* a max_rows below the rows held: SAGEICP_ERR_INVALID */
int sageicp_map_archive_info(const sageicp_map *m, sageicp_archive_info *out);
int sageicp_map_archive_clear(sageicp_map *m);
int sageicp_map_archive_voxels(const sageicp_map *m, uint64_t first, sageicp_archive_voxel *out, uint64_t cap, uint64_t *n_out);
int sageicp_map_archive_rows(const sageicp_map *m, int which, uint64_t first, double *out_xyzl, uint64_t cap, uint64_t *n_out);
int sageicp_map_archive_rows_device(const sageicp_map *m, int which, uint64_t first, const sageicp_device_points *dst,
                                    void *stream /* hipStream_t; NULL = null stream */, uint64_t *n_out);
int sageicp_map_archive_msg(const sageicp_map *m, int which, uint64_t first, const sageicp_msg_colors *colors, void *out,
                            uint64_t cap_points, uint64_t *n_out);
int sageicp_map_archive_msg_device(const sageicp_map *m, int which, uint64_t first, const sageicp_msg_colors *colors, void *out,
                                   uint64_t cap_points, void *stream /* hipStream_t; NULL = null stream */, uint64_t *n_out);
int sageicp_pipeline_set_archive(sageicp_pipeline *p, int enable, uint64_t max_rows);   /* its map's */

/* ---- recall: a place of the session's map back into a map that can be searched -------------------------
 * Additions only; the ABI version stays.  The session's voxels of `src` are the SAGEICP_ARCHIVE_LATEST records of its
 * archive in log order followed by its live voxels in sageicp_map_pointcloud's order (what SAGEICP_SESSION exports; with
 * the archive off or empty, the live map).  sageicp_map_recall keeps voxel v iff its FIRST stored row p is not far from
 * `center` — far as RemovePointsFarFromLocation decides it, (p - center).squaredNorm() > radius * radius, radius * radius
 * formed once; a voxel is kept or dropped whole, by its first row alone — and puts the kept voxels into `dst` in session
 * order, each with its rows bit for bit in stored order: what a local map of max_distance = radius standing at `center`
 * would still hold of the session.
 * dst: cleared first, as by sageicp_map_clear (its own archive is left alone and nothing is logged into it); afterwards
 * it holds the kept voxels and nothing else, blocks handed out in arrival order (sageicp_map_pointcloud: the kept rows in
 * session order), and it is resident: filled on the device, nothing downloaded.  From then on an ordinary map — search,
 * updates on either side, archive, exports, download.  Its rows, their order and its counters equal those of a fresh map
 * of the same voxel size and policy after sageicp_map_add_points(SESSION rows) and sageicp_map_remove_far(center) at
 * max_distance = radius; where a region lies in the point array and a slot in the table may differ (no result depends on
 * either), and so may the block a LATER update gives a new voxel: here every block below num_voxels is taken, there the
 * evicted ones are free and handed out first.
 * SAGEICP_ERR_INVALID, dst untouched: a null handle; dst == src; a non-finite centre; a radius that is negative or NaN
 * (+inf recalls the whole session); a dst whose voxel size, points per voxel (basic, critical) or basic labels differ
 * from src's; a dst in reference-order mode, spanning several devices, or on another device than src's first.  src may be
 * in either mode and span several devices (its first copy is the one that archives).  Device work: SAGEICP_ERR_NO_DEVICE
 * without one.  SAGEICP_ERR_CAPACITY: more than 2^32 - 2 records, or more voxels / storage units than a map holds.  After
 * any failure past the argument checks dst is left cleared, never partly filled.  src: a pending host tail of its archive
 * is moved to the device first, as by an export; a resident src stays resident.  Synchronous. */
typedef struct sageicp_recall_info {
    uint64_t voxels, rows;                    /* what dst holds now */
    uint64_t archive_voxels, archive_rows;    /* of them, from the archive (LATEST) */
    uint64_t map_voxels, map_rows;            /* of them, from src's live map */
    uint64_t session_voxels, session_rows;    /* what was considered */
} sageicp_recall_info;
int sageicp_map_recall(const sageicp_map *src, const double center[3], double radius, sageicp_map *dst,
                       sageicp_recall_info *info /* may be NULL */);
int sageicp_pipeline_recall(const sageicp_pipeline *p, const double center[3], double radius, sageicp_map *dst,
                            sageicp_recall_info *info /* may be NULL */);   /* its local map's */

/* ---- loop closure: a closure spread over the trajectory, the session's map re-posed -------------------
 * Additions only; the ABI version stays; off unless called: no other entry does anything it did not do before, and a
 * pipeline's own state (its poses, its local map) is never touched — it keeps running in its odometry frame.
 *
 * Corrections (host, fp64, no device).  poses: n rows T_world_k, (qx, qy, qz, qw, tx, ty, tz).  closed: where pose j really
 * is, in pose i's frame of the world — what sageicp_relocalize returns against a map recalled around pose i.
 *     delta = closed * poses[j]^-1          (se3_mul, se3_inv; REP-105's map->odom transform after the closure)
 *     c     = t_j, the translation of poses[j]: the pivot
 *     alpha_k = 0 for k <= i, 1 for k >= j, between them the share of path length
 *               sum_{m=i+1..k} |t_m - t_{m-1}| / sum_{m=i+1..j} |t_m - t_{m-1}|  ((k - i) / (j - i) if the whole path is 0)
 *     C_k   = Tr(c) * exp(alpha_k * log(Tr(-c) * delta * Tr(c))) * Tr(-c)          (se3_log, se3_exp)
 *     poses_out[k] = C_k * poses[k]
 * Interpolating about t_j makes the result move with the trajectory when the trajectory is translated.  The two ends do
 * not pass through log or exp: for k <= i, C_k is (0,0,0,1,0,0,0) and poses_out[k] is poses[k], bit for bit; for k >= j,
 * C_k is delta's own bytes.  info: delta, its rotation angle (rad), shift = how far pose j moves (|closed.t - t_j|), path =
 * the path length from pose i to pose j.  SAGEICP_ERR_INVALID, nothing written: a null pointer that is not optional;
 * n == 0, i >= j, j >= n; a non-finite input; a quaternion of norm 0; a delta that turns by more than pi - 1e-6 (that is
 * not drift, and the logarithm is not to be trusted there).  Several closures are applied one after another
 * (poses_out of one is poses of the next, and the corrections compose: C'_k * C_k); a pose graph with many simultaneous
 * constraints is out of scope.
 *
 * Stays (device).  The session's voxels of `which` are enumerated as recall enumerates them: SAGEICP_ARCHIVE_ALL every
 * record in log order; SAGEICP_ARCHIVE_LATEST the LATEST records in log order; SAGEICP_SESSION those, then the live
 * voxels in sageicp_map_pointcloud's order.  positions: n >= 1 rows (x, y, z), the sensor position of the call with serial
 * s (sageicp_archive_voxel.update).  A voxel is evicted by its FIRST row p alone, so between its insertion and its
 * eviction no position was far from p — far as RemovePointsFarFromLocation decides it, (p - position).squaredNorm() >
 * max_distance * max_distance.  With hi = min(update, n) - 1 for a record and n - 1 for a live voxel, walk k = hi, hi - 1,
 * ... while k >= 0 and positions[k] is not far from p: stay = the walked k of smallest squared distance, the larger k on
 * a tie; max(hi, 0) if nothing was walked.  This is not the nearest pose over all poses: on an out-and-back drive that is
 * often one of the old pass, whose correction is the wrong one.  One uint32 per voxel of the selection, in selection
 * order; `first` skips voxels, *n_out = the voxels of the selection, [first, first + min(cap, *n_out - first)) written.
 *
 * The re-posed export (device).  The rows of the selection, in the order of sageicp_map_archive_rows(which), each moved
 * by corrections[stay of its voxel] — the point action of sageicp_transform_points, bit for bit; the label untouched —
 * and then converted to the caller's layout; first, cap, *n_out, stream and lifetime rules, refusals, and "leaves a
 * resident map resident" as sageicp_map_archive_rows[_device].  With every correction the identity the bytes are those
 * of the plain export (a coordinate that is -0.0 leaves as +0.0, as it does through sageicp_transform_points).
 * SAGEICP_ERR_INVALID: a null argument, a `which` that is none of the three, n == 0 or beyond 2^32 - 1, a non-finite
 * position or correction.  SAGEICP_ERR_NO_DEVICE without a device; SAGEICP_ERR_CAPACITY beyond 2^32 - 2 records or rows.
 *
 * The pipeline's entries take the poses and the positions from the pipeline (j: its last pose; n must be its number of
 * poses) and return SAGEICP_ERR_INVALID unless the archive's `updates` equals sageicp_pipeline_num_poses — the archive on
 * from the first frame and nothing interrupting the count: only then is serial s pose s. */
typedef struct sageicp_closure_info {
    double delta[7];
    double angle;
    double shift;
    double path;
    uint64_t i, j;
} sageicp_closure_info;
int sageicp_closure_corrections(const double *poses /* n x 7 */, uint64_t n, uint64_t i, uint64_t j, const double closed[7],
                                double *corrections_out /* n x 7 */, double *poses_out /* n x 7, may be NULL */,
                                sageicp_closure_info *info /* may be NULL */);
int sageicp_map_session_stays(const sageicp_map *m, int which, uint64_t first, const double *positions /* n x 3 */, uint64_t n,
                              uint32_t *stay_out, uint64_t cap, uint64_t *n_out);
int sageicp_map_session_corrected(const sageicp_map *m, int which, uint64_t first, const double *positions /* n x 3 */,
                                  const double *corrections /* n x 7 */, uint64_t n, double *out_xyzl, uint64_t cap,
                                  uint64_t *n_out);
int sageicp_map_session_corrected_device(const sageicp_map *m, int which, uint64_t first, const double *positions,
                                         const double *corrections, uint64_t n, const sageicp_device_points *dst,
                                         void *stream /* hipStream_t; NULL = null stream */, uint64_t *n_out);
int sageicp_pipeline_closure(const sageicp_pipeline *p, uint64_t i, const double closed[7], double *corrections_out,
                             double *poses_out /* may be NULL */, sageicp_closure_info *info /* may be NULL */);
int sageicp_pipeline_session_corrected(const sageicp_pipeline *p, int which, uint64_t first, const double *corrections,
                                       uint64_t n, double *out_xyzl, uint64_t cap, uint64_t *n_out);
int sageicp_pipeline_session_corrected_device(const sageicp_pipeline *p, int which, uint64_t first, const double *corrections,
                                              uint64_t n, const sageicp_device_points *dst,
                                              void *stream /* hipStream_t; NULL = null stream */, uint64_t *n_out);

/* ---- session rebuild: the corrected session voxelised again, into a map that can be searched ---------------
 * Additions only; the ABI version stays; off unless called.  sageicp_map_session_corrected* returns rows: a street driven
 * twice is in them twice, and rows cannot be searched.  sageicp_map_session_rebuild puts them through the map's own
 * retention policy on the device and leaves a map.  Afterwards dst equals a fresh map of dst's voxel size and policy after
 *   1. sageicp_map_add_points of the rows sageicp_map_session_corrected(src, which, 0, positions, corrections, n, ..)
 *      returns, in that order, and
 *   2. if `center` is given, sageicp_map_remove_far(center) at max_distance = radius — far as RemovePointsFarFromLocation
 *      decides it, (p - center).squaredNorm() > radius * radius on the voxel's first stored row p, radius * radius formed once:
 * the bytes and the order of sageicp_map_pointcloud (kept voxels in the order of their first arrival), sageicp_map_size and
 * sageicp_map_num_voxels are the same, every later search gives the same answer and every later update behaves the same —
 * where a region lies in the point array and a slot in the table may differ (no result depends on either), and so may
 * the block a LATER update gives a new voxel: here every block below num_voxels is taken, there the evicted ones are free
 * and handed out first (recall's caveat).  Unlike recall's, the voxels are new ones: a moved row is keyed by
 * static_cast<int>(coordinate / voxel_size) of its MOVED coordinates, so the rows of one source voxel may land in several
 * destination voxels; rows of source voxels of different passes and generations (SAGEICP_ARCHIVE_ALL) land in one, where
 * they go through VoxelBlock::AddPoint in arrival order; and the crop is decided by the destination voxel's FINAL first
 * stored row, which may be a later arrival that replaced an unlabelled first one.
 * dst: cleared first, as by sageicp_map_clear (its own archive is left alone and nothing is logged into it; its own
 * max_distance is unchanged), and it ends resident: filled on the device, nothing downloaded; from then on an ordinary map.
 * info: what dst holds; the selection (what was moved and keyed); what the retention policy kept of it, before the crop;
 * and built - held.
 * SAGEICP_ERR_INVALID, dst untouched: dst's refusals are recall's (a null handle, dst == src, a dst whose voxel size,
 * points per voxel or basic labels differ from src's, a dst in reference-order mode, spanning several devices or on
 * another device than src's first) and more than 32 basic labels; src, which, positions, corrections and n have the
 * refusals of sageicp_map_session_corrected; with a centre, a non-finite centre and a radius that is negative or NaN
 * (center == NULL: everything is kept and radius is not looked at).  Device work: SAGEICP_ERR_NO_DEVICE without one.
 * Found on the device: SAGEICP_ERR_INVALID, a moved coordinate that is not finite; SAGEICP_ERR_CAPACITY, a moved row's voxel
 * index beyond +-2^20, more than 2^32 - 2 records or rows, more voxels / storage units than a map holds.  After any failure
 * past the argument checks dst is left cleared and usable, never partly filled.  src is read as by the corrected export: a
 * pending host tail of its archive is moved to the device first, a resident src stays resident.  Synchronous; the same
 * bytes on every run.  The pipeline's entry takes the positions from the pipeline (n must be its number of poses) and
 * returns SAGEICP_ERR_INVALID unless the archive's `updates` equals sageicp_pipeline_num_poses, as the closure entries do. */
typedef struct sageicp_rebuild_info {
    uint64_t voxels, rows;                  /* what dst holds now */
    uint64_t session_voxels, session_rows;  /* the selection: what was moved and keyed */
    uint64_t built_voxels, built_rows;      /* after the retention policy, before the crop */
    uint64_t cropped_voxels, cropped_rows;  /* built - held */
} sageicp_rebuild_info;
int sageicp_map_session_rebuild(const sageicp_map *src, int which, const double *positions /* n x 3 */,
                                const double *corrections /* n x 7 */, uint64_t n,
                                const double center[3] /* NULL: keep everything, radius ignored */, double radius,
                                sageicp_map *dst, sageicp_rebuild_info *info /* may be NULL */);
int sageicp_pipeline_session_rebuild(const sageicp_pipeline *p, int which, const double *corrections /* n x 7 */, uint64_t n,
                                     const double center[3] /* NULL: keep everything */, double radius, sageicp_map *dst,
                                     sageicp_rebuild_info *info /* may be NULL */);

/* ---- pose graph: several loop closures at once -------------------------------------------------------------
 * Additions only; the ABI version stays; off unless called.  sageicp_closure_corrections spreads ONE closure; applied one
 * after another, a later closure reopens the seam of an earlier one.  This is the optimiser between Relocalize's relative
 * poses and sageicp_map_session_corrected*: a chain of odometry edges plus c <= 256 closures, minimised together.
 *
 * The problem.  poses: n >= 2 rows x_k = T_world_k, (qx, qy, qz, qw, tx, ty, tz), unit quaternions.  The tangent is
 * (upsilon, omega), translation first.  Odometry edges are implicit: for k < n - 1, Z_k = poses[k]^-1 * poses[k + 1], with
 * information odom_info, a row-major symmetric positive definite 6x6 — one for all edges (odom_info_stride 0) or one per
 * edge (36).  Closure edges are explicit, in any order, several on one pair allowed: z = T_a_b (pose b in pose a's frame),
 * a != b.  With
 *     r_e(x) = log(Z_e^-1 * x_a^-1 * x_b)          F(x) = sum_e r_e^T info_e r_e
 * F is minimised over the poses but `anchor`, by Gauss-Newton with the exact Jacobians (d r / d delta_b = Jr^-1(r),
 * d r / d delta_a = -Jr^-1(r) Ad((x_a^-1 x_b)^-1)) under the update x_k <- x_k * exp(delta_k) (quaternion renormalised), from
 * `initial` (NULL: poses).  Every term is a function of relative transforms (x_a^-1 x_b is formed from t_b - t_a), so the
 * problem moves with the trajectory at UTM coordinates.  The step solves H delta = -g, H = sum J^T info J, exactly (a block
 * tridiagonal factor plus a rank-6c correction, refined twice against the edges' own blocks); it is tried at s = 1, 1/2, ...
 * (max_halvings halvings) and taken only if F decreases — the full step also where F cannot tell, within (edges + 64) 2^-52 F
 * of no change, what two evaluations of F at one point may differ by, and never above F at the start.  status: 0 an accepted step with |s delta|_inf <= step_tol; 1 no trial decreased F (the floating-point floor);
 * 2 max_iterations reached.  The anchor's output is its input bit for bit and its correction (0,0,0,1,0,0,0).
 *     corrections_out[k] = poses_out[k] * poses[k]^-1       (sageicp_closure_corrections' convention: it goes straight
 *                                                            into sageicp_map_session_corrected*)
 * info: F at the start and at poses_out, grad_max = |dF/d delta|_inf at poses_out, step_last = |s delta|_inf of the last
 * accepted step, max_shift = the largest |t_out - t_poses|, accepted iterations, halvings in all, status, where it ran.
 * where: 1 the host (sequential block Thomas), 2 the device (block cyclic reduction; the same bytes on
 * every run; SAGEICP_ERR_NO_DEVICE without one), 0 the device from SAGEICP_GRAPH_AUTO_POSES poses on if there is one.
 * Host and device agree to tolerance, not to bits.  The device path takes the current device and works in buffers of
 * its own for the call: per pose about 2.6 KB, plus at most 512 MiB (or one column, if that is more) for the
 * right-hand sides, which are solved in chunks of columns.
 * SAGEICP_ERR_INVALID, nothing written: a null pointer that is not optional; n < 2; a == b or an index >= n; anchor >= n;
 * a non-finite input; a quaternion of norm 0; an info that is not symmetric to the bit or not positive definite by an
 * unpivoted Cholesky; a stride that is neither 0 nor 36; where > 2; a step_tol that is negative or NaN; a chain whose
 * normal matrix the factor finds not positive definite to fp64 (hundreds of thousands of metre steps with few closures).
 * SAGEICP_ERR_CAPACITY: c > 256, or n beyond 2^31.
 * sageicp_graph_edge_from_closed: the edge of "pose j really is at `closed`, in pose i's frame of the world"
 * (sageicp_closure_corrections' argument; what Relocalize returns against a map recalled around pose i): z = poses[i]^-1 *
 * closed, a = i, b = j.  sageicp_graph_cost: F at `at` (host, fp64), and each edge's term (odometry first).
 * The pipeline's entry takes the pipeline's poses; the pipeline itself is not touched. */
#define SAGEICP_GRAPH_AUTO_POSES 4000
typedef struct sageicp_graph_edge {
    uint64_t a, b;
    double z[7];
    double info[36];
} sageicp_graph_edge;
typedef struct sageicp_graph_params {
    uint64_t anchor;            /* default 0 */
    uint32_t max_iterations;    /* default 50 */
    uint32_t max_halvings;      /* default 10 */
    double step_tol;            /* default 1e-9 */
    uint32_t where;             /* 0 auto, 1 host, 2 device */
    uint32_t reserved;
} sageicp_graph_params;
typedef struct sageicp_graph_info {
    double cost_initial, cost_final, grad_max, step_last, max_shift;
    uint32_t iterations, halvings, status, where;
} sageicp_graph_info;
void sageicp_graph_params_default(sageicp_graph_params *p);
int sageicp_graph_edge_from_closed(const double *poses /* n x 7 */, uint64_t n, uint64_t i, uint64_t j, const double closed[7],
                                   const double info[36], sageicp_graph_edge *out);
int sageicp_graph_cost(const double *poses /* n x 7 */, uint64_t n, const double *odom_info, uint32_t odom_info_stride,
                       const sageicp_graph_edge *closures, uint32_t c, const double *at /* n x 7 */, double *cost,
                       double *per_edge /* n - 1 + c, may be NULL */);
int sageicp_graph_optimize(const double *poses /* n x 7 */, uint64_t n, const double *odom_info, uint32_t odom_info_stride,
                           const sageicp_graph_edge *closures /* may be NULL if c == 0 */, uint32_t c,
                           const double *initial /* n x 7; NULL = poses */, const sageicp_graph_params *params /* NULL = defaults */,
                           double *poses_out /* n x 7 */, double *corrections_out /* n x 7, may be NULL */,
                           sageicp_graph_info *info /* may be NULL */);
int sageicp_pipeline_graph_optimize(const sageicp_pipeline *p, const double *odom_info, uint32_t odom_info_stride,
                                    const sageicp_graph_edge *closures, uint32_t c, const sageicp_graph_params *params,
                                    double *corrections_out /* n x 7 */, double *poses_out /* may be NULL */,
                                    sageicp_graph_info *info /* may be NULL */);

/* ---- robust pose graph: false closures down-weighted; an edge's information from a quality report --------
 * Additions only; the ABI version stays.  One false place match among the closures wrecks a least-squares optimum.  With a
 * robust kernel every CLOSURE's term s = r^T info r enters F as rho(s) (odometry edges stay quadratic), c = scale:
 *     HUBER   rho = s if s <= c^2, else 2 c sqrt(s) - c^2      weight rho' = 1 if s <= c^2, else c / sqrt(s)
 *     CAUCHY  rho = c^2 log1p(s / c^2)                          weight 1 / (1 + s / c^2)
 *     GM      rho = c^2 s / (c^2 + s)                           weight (c^2 / (c^2 + s))^2
 * Huber bounds a false closure's pull, it does not reject it; Cauchy and Geman-McClure redescend.  The step is Gauss-Newton
 * on the re-weighted edges (each closure's linearisation scaled by sqrt(rho')): g is the exact gradient of F, H stays
 * positive definite.  Backtracking, the (edges + 64) 2^-52 F rule and the stop rule are sageicp_graph_optimize's, applied to
 * the robust F, on the host and on the device alike.  scale is a chi-square threshold in the edge's own information, which
 * therefore has to be a real one: sageicp_graph_info_from_quality below.
 * anneal = 1: from a drifted start the TRUE closures lie far outside c^2 too and a redescending kernel would give them up.
 * With s0 the largest closure term at the start (evaluated on the host), the call runs the stages c^2 f^m, ..., c^2 f, c^2
 * (f = anneal_factor; m the smallest count with c^2 f^m >= s0, so one stage if s0 <= c^2; more than 1024 stages:
 * SAGEICP_ERR_CAPACITY), each but the last for at most stage_iterations iterations (fewer on status 0 or 1), the last under
 * max_iterations; its status is the call's.  iterations and halvings count all stages.
 * cost_initial and cost_final are the FINAL kernel's F (scale c) at the start and at poses_out; cost_final <= cost_initial is
 * promised only with anneal == 0.  grad_max is the gradient of that F.  closure_chi2_out[k] is the raw s of closure k at
 * poses_out (sageicp_graph_cost's term), closure_weight_out[k] its rho' at c^2; outliers counts weights below 0.5: drop
 * those matches.  robust == NULL or kernel NONE: sageicp_graph_optimize itself, bit for bit, weights 1, stages 1.
 * SAGEICP_ERR_INVALID, nothing written, besides sageicp_graph_optimize's: kernel > 3; anneal > 1; a scale or anneal_factor
 * that is not finite; scale <= 0; anneal_factor <= 1; stage_iterations == 0.
 *
 * sageicp_graph_info_from_quality: the information of the edge sageicp_graph_edge_from_closed makes of `closed`, from the
 * quality report AT closed (what sageicp_relocalize returns).  The report's tangent is the left perturbation closed <-
 * exp(xi) closed, an edge's the right one z <- z exp(eta), z = poses[i]^-1 closed: xi = Ad(closed) eta whatever poses[i], so
 *     info = gain * Ad(closed)^T (JTJ / s2) Ad(closed),  Ad(T) = [[R, hat(t) R], [0, R]],  s2 = sum_w_r2 / (3 n_pairs - 6),
 * symmetrised as (M + M^T) / 2.  gain > 0 is the caller's noise model: ICP covariances are overconfident (they know the
 * pairs' noise, not the wrong pairs), so a gain well below 1 is usual.  SAGEICP_ERR_INVALID, nothing written: a null
 * argument; covariance_valid == 0; s2 not above 0; an input that is not finite; a quaternion of norm 0; gain not above 0; a
 * result that is not positive definite by the optimiser's own test (UTM coordinates: register in a local frame). */
#define SAGEICP_GRAPH_KERNEL_NONE 0
#define SAGEICP_GRAPH_KERNEL_HUBER 1
#define SAGEICP_GRAPH_KERNEL_CAUCHY 2
#define SAGEICP_GRAPH_KERNEL_GM 3
typedef struct sageicp_graph_robust {
    uint32_t kernel, anneal;          /* anneal: 0 / 1 */
    double scale;                     /* c > 0; default sqrt(16.81): chi-square, 6 dof, 99 % */
    double anneal_factor;             /* > 1, default 2 */
    uint32_t stage_iterations;        /* >= 1, default 3 */
    uint32_t reserved;
} sageicp_graph_robust;
typedef struct sageicp_graph_robust_info {
    double scale2_first;              /* c^2 of the first stage */
    uint32_t stages, outliers;        /* outliers: closures with weight < 0.5 at poses_out */
} sageicp_graph_robust_info;
void sageicp_graph_robust_default(sageicp_graph_robust *r);
int sageicp_graph_optimize_robust(const double *poses /* n x 7 */, uint64_t n, const double *odom_info, uint32_t odom_info_stride,
                                  const sageicp_graph_edge *closures, uint32_t c, const double *initial,
                                  const sageicp_graph_params *params, double *poses_out, double *corrections_out,
                                  sageicp_graph_info *info, const sageicp_graph_robust *robust /* NULL = none */,
                                  double *closure_chi2_out /* c, may be NULL */, double *closure_weight_out /* c, may be NULL */,
                                  sageicp_graph_robust_info *rinfo /* may be NULL */);
int sageicp_pipeline_graph_optimize_robust(const sageicp_pipeline *p, const double *odom_info, uint32_t odom_info_stride,
                                           const sageicp_graph_edge *closures, uint32_t c, const sageicp_graph_params *params,
                                           double *corrections_out /* n x 7 */, double *poses_out /* may be NULL */,
                                           sageicp_graph_info *info /* may be NULL */, const sageicp_graph_robust *robust,
                                           double *closure_chi2_out, double *closure_weight_out, sageicp_graph_robust_info *rinfo);
int sageicp_graph_info_from_quality(const sageicp_quality *q, const double closed[7], double gain, double info_out[36]);

/* ---- place recognition: the semantic scan context of key frames (place.hip) -------------------------------------------
 * Additions only; the ABI version stays.  A descriptor says where the sensor stood: a polar grid of R rings by S sectors
 * around it that holds, per cell, the highest return (a byte) and the most important class.  Descriptors of one
 * parameter set are kept in a database on the device, and a new one is matched against all of them under all S
 * rotations by counting the cells that agree.  Everything that decides a byte or a rank is an integer or a plain fp64
 * comparison against two tables made once on the host, so the same input gives the same bytes and the same matches on
 * every run.
 *
 * Parameters.  Refused with SAGEICP_ERR_INVALID (before any device is asked): a double that is not finite,
 * min_range <= 0 or min_range >= max_range, z_lo >= z_hi, rings outside [1, 64], sectors outside [3, 360],
 * rings * sectors > 16384 (two u32 planes of that many cells are what one workgroup's LDS holds).
 * Tables (sageicp_place_tables, host code, no device):
 *     edge2[k] = e * e,  e = min_range + k * ((max_range - min_range) / rings),  k = 0 .. rings    (fp64, this association)
 *     dir[s]   = (cos(a), sin(a)),  a = (2.0 * M_PI * s) / sectors,  s = 0 .. sectors - 1           (the host's libm)
 * A row (x, y, z, l), all fp64 without contraction:
 *   class   c = l truncated toward zero; the row is ignored unless -1 < l < 256 (so c is 0 .. 255; -0.5 is class 0) and
 *           rank[c] != 0 — a rank of 0 is how the caller drops moving classes and unlabelled points.
 *   ring    r2 = x * x + y * y; ignored when r2 < edge2[0] or r2 >= edge2[rings]; otherwise the ring is the number of
 *           k in 1 .. rings - 1 with r2 >= edge2[k].  No square root is taken.
 *   sector  f(s) = (dir[s].x * y - dir[s].y * x >= 0); the sector is the s with f(s) true and f((s + 1) % sectors)
 *           false.  No atan2 decides anything (the kernel guesses with one in fp32, then steps with f).
 *   height  t = (z - z_lo) / (z_hi - z_lo); v = t > 0 ? (t < 1 ? t : 1) : 0; h = 1 + (int)floor(v * 254.0): 1 .. 255,
 *           0 means empty.
 *   key     rank[c] << 8 | c.
 * Per cell the descriptor keeps the maximum h and the low byte of the maximum key (the class of highest rank, ties to
 * the higher class number); the two planes are independent.  It leaves as 2 * rings * sectors bytes: the height plane
 * [rings][sectors], then the class plane [rings][sectors].  n == 0: all zeros.  A coordinate that is not finite refuses
 * the call (labels are not checked: a label that is not finite is a row ignored). */
typedef struct sageicp_place_params {
    double min_range, max_range;       /* metres in the sensor's xy plane: min_range <= r < max_range */
    double z_lo, z_hi;                 /* the heights mapped to bytes 1 and 255 */
    int32_t rings, sectors;            /* R in [1, 64], S in [3, 360], R * S <= 16384 */
    uint8_t rank[256];                 /* per class: 0 = ignored, otherwise its importance */
} sageicp_place_params;                                            /* 296 bytes, doubles first, no padding */
int sageicp_place_tables(const sageicp_place_params *params, double *edge2_out /* [rings + 1] */,
                         double *dir_out /* [sectors][2] */);
int sageicp_place_describe(const double *xyzl, uint64_t n, const sageicp_place_params *params,
                           uint8_t *desc_out /* 2 * rings * sectors bytes */, int device);
/* the same of a frame in device memory: the layout and caller-memory checks of sageicp_occupancy_grid_device, on the
 * device the frame lives on and behind the work on `stream`; the bytes go to host memory.  Synchronous. */
int sageicp_place_describe_device(const sageicp_device_frame *frame, const sageicp_place_params *params,
                                  uint8_t *desc_out /* host */, void *stream /* hipStream_t; NULL = null stream */);

/* The database: descriptors of one parameter set as [N][2][rings][sectors] bytes in device memory (it grows by
 * doubling, from 64 entries, on the handle's stream; N <= 2^20, beyond: SAGEICP_ERR_CAPACITY), each with a tag and a
 * pose (qx qy qz qw tx ty tz) kept on the host.  Every entry is synchronous.  _read returns what _add was given, byte for
 * byte (any of its three outputs may be NULL), so a database is saved by _read and loaded by _add.
 *
 * sageicp_place_db_match(db, desc, query, out, n_out).  For entry e and shift k in 0 .. S - 1, agree(k) is the number of
 * cells (r, s) with: the query's height at (r, s) > 0, the entry's height at (r, (s + k) % S) > 0, the two class bytes
 * equal, and the absolute height difference <= h_tol.  shift is the smallest k of maximal agree and agree that
 * maximum; n_query and n_entry are the occupied-cell counts, m = max(n_query, n_entry), and
 * similarity = m ? (double)agree / (double)m : 0.0 (one division).  Only entries with index < size - exclude_last are
 * considered (exclude_last >= size: *n_out = 0).  Ranking: a precedes b when agree_a * m_b > agree_b * m_a, exact in
 * u64; an entry with m == 0 ranks as 0; ties go to the lower index.  The first top_k are taken, then those with
 * similarity < min_similarity are dropped; *n_out tells how many were written.  Brute force: every considered entry is
 * scored under every shift, so the answer is exact.  Refused (SAGEICP_ERR_INVALID): top_k outside [1, 16], h_tol > 255,
 * a min_similarity that is not finite.
 * Convention.  A query sensor turned by +yaw about z relative to the entry's sensor sees the entry's sector s + k in its
 * own sector s, so T_world_query ~ T_world_entry o R_z(yaw): with w = 2.0 * M_PI / S, yaw = shift * w when
 * shift <= S / 2 (integer division) and (shift - S) * w otherwise (both integer to double, then one product), and
 * prior = (q_entry (x) q_z(yaw), t_entry) — the Hamilton product, not renormalised, q_z as at
 * sageicp_relocalize_candidates; a shift of 0 leaves the entry's bits.  prior goes straight into sageicp_relocalize.
 * sageicp_place_prior is that rule alone (host code, no device; SAGEICP_ERR_INVALID for a shift >= sectors). */
typedef struct sageicp_place_db sageicp_place_db;
typedef struct sageicp_place_query {
    double min_similarity;
    uint64_t exclude_last;             /* the newest entries are not considered (a typical value: some tens) */
    uint32_t top_k, h_tol;             /* 1 .. 16; 0 .. 255 */
} sageicp_place_query;                                             /* 24 bytes */
typedef struct sageicp_place_match {
    double similarity, yaw;
    double pose[7], prior[7];          /* the entry's pose; the prior for sageicp_relocalize */
    uint64_t index, tag;
    uint32_t agree, n_query, n_entry, shift;
} sageicp_place_match;                                             /* 160 bytes, doubles first, no padding */
sageicp_place_db *sageicp_place_db_create(const sageicp_place_params *params, int device);
void sageicp_place_db_destroy(sageicp_place_db *db);
uint64_t sageicp_place_db_size(const sageicp_place_db *db);
int sageicp_place_db_clear(sageicp_place_db *db);
int sageicp_place_db_add(sageicp_place_db *db, const uint8_t *desc /* host bytes */, uint64_t tag,
                         const double pose[7] /* NULL = identity */, uint64_t *index_out /* optional */);
int sageicp_place_db_read(const sageicp_place_db *db, uint64_t first, uint64_t count, uint8_t *desc_out,
                          uint64_t *tags_out, double *poses_out /* [count][7] */);
int sageicp_place_db_match(const sageicp_place_db *db, const uint8_t *desc /* host bytes */,
                           const sageicp_place_query *query, sageicp_place_match *out /* [top_k] */, uint32_t *n_out);
int sageicp_place_prior(const double pose[7], uint32_t shift, int32_t sectors, double *yaw_out, double prior_out[7]);

/* In the pipeline (off by default; off, no kernel, launch or result changes).  For every frame that becomes a key frame
 * the pipeline, after the key-frame decision and outside the times the register calls report, (1) describes the RAW
 * frame (the copy key-frame selection sets aside), (2) matches the descriptor against the database BEFORE adding it,
 * with the given query, and (3) appends it device to device with tag = key_frame_index and pose = key_pose.  Other
 * frames leave described = 0 and n_matches = 0.  The only host synchronisation added is the one download of the match
 * records.  sageicp_pipeline_set_places is refused with SAGEICP_ERR_INVALID while key-frame selection is off;
 * switching key frames off (or setting them anew) switches places off.  Switching places on starts an empty database.
 * sageicp_pipeline_reinitialize keeps the database, as it keeps the key-frame state: tags then refer to the earlier
 * trajectory.  sageicp_pipeline_place_reset and sageicp_pipeline_key_frame_reset clear it.  A register call that fails
 * changes nothing in the database.  sageicp_pipeline_place_db returns the pipeline's database, borrowed (NULL while
 * places are off): valid until places are switched off or the pipeline goes. */
typedef struct sageicp_place_info {
    sageicp_place_match matches[16];
    uint64_t entries;                  /* the database's size */
    int32_t enabled;
    int32_t described;                 /* the last frame registered was a key frame and was described */
    uint32_t n_matches, reserved;
} sageicp_place_info;                                              /* 2584 bytes */
int sageicp_pipeline_set_places(sageicp_pipeline *p, int enable, const sageicp_place_params *params,
                                const sageicp_place_query *query);
int sageicp_pipeline_place_info(const sageicp_pipeline *p, sageicp_place_info *out);
const sageicp_place_db *sageicp_pipeline_place_db(const sageicp_pipeline *p);
int sageicp_pipeline_place_reset(sageicp_pipeline *p);

/* ---- KITTI trajectory metrics: sage_icp::metrics (metrics/Metrics.hpp:33-37) ----------------------
 * Host-only (the reference's are CPU code too).  Poses are 4x4 homogeneous matrices, ROW-major
 * (a KITTI poses.txt row padded with 0 0 0 1), n of them, 16 doubles each.
 * sageicp_metrics_seq_error: SeqError, Metrics.cpp:140-155 — KITTI devkit relative error over
 *   segments of 100..800 m starting every 10th frame: (translation %, rotation deg/100 m with
 *   the reference's 180/3.14).  NaN when no segment is long enough, as in the reference.
 * sageicp_metrics_absolute_trajectory_error: AbsoluteTrajectoryError, Metrics.cpp:157-191 — RMSE
 *   of the rotation angle [rad] and of the translation [m] after a rigid Umeyama alignment. */
int sageicp_metrics_seq_error(const double *poses_gt, const double *poses_result, uint64_t n,
                              float *avg_trans_error, float *avg_rot_error);
int sageicp_metrics_absolute_trajectory_error(const double *poses_gt, const double *poses_result,
                                              uint64_t n, float *ate_rot, float *ate_trans);

#ifdef __cplusplus
}
#endif
#endif /* SAGEICP_H_ */
