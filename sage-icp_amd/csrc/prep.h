// The per-frame driver in front of registration: what a frame is prepared from (FrameSource: host rows, a device frame,
// a message), what it passes through (deskew, the dynamic vehicle filter) and the buffers of one preparation (Prep).
// Declarations only: Prep's bodies are in prep.hip, DynFilter's in dyn_filter.hip.  Included by capi_internal.h; not part of
// the C ABI.
#pragma once

#include "replay_pool.h"

namespace sageicp {

struct DynFilterConfig {
    double dy_th = 0.5;
    std::vector<uint32_t> dynamic_labels;      // the reference's std::vector<int>, compared as uint32_t
    std::vector<uint32_t> landmark_labels;
};

// buffers of one Prep; run() filters a frame already on the device (n points at `in`) into `out` (may be `in`),
// passing the cropped points through `tmp` (n points)
struct DynFilter {
    size_t cap = 0;                            // points the buffers of reserve() hold (all of them: 0 after a failed reserve)
    DevBuf<uint32_t> d_labels, d_ctr;
    PinnedBuf<uint32_t> h_ctr;                 // [0..3] counters, [4] flags
    DevBuf<unsigned long long> d_cnt, d_pos, d_vkey, d_lkey, d_count;
    DevBuf<float4> d_vp, d_vs, d_lp, d_ls;
    DevBuf<uint32_t> d_vval, d_lval, d_vframe, d_parent, d_root, d_size, d_rec_of_root, d_start, d_rkv, d_off;
    DevBuf<uint4> d_rec;
    DevBuf<unsigned char> d_temp;
    PinnedBuf<uint4> h_rec;                    // the component table
    PinnedBuf<uint32_t> h_off;                 // output offset per component (~0: dropped)
    OwnedEvent ev[6];                          // device time of the three launch batches (sageicp_set_profiling)
    OwnedEvent ev_table;
    std::vector<uint32_t> order_scratch, size_scratch;
    sageicp_dynfilter_info info{};             // of the last run

    int reserve(size_t n, size_t nlabels);
    int run(const Point4 *in, uint64_t n, double max_range, double min_range, double label_max_range,
            const DynFilterConfig &cfg, Point4 *tmp, Point4 *out, int *d_ovf, uint64_t &n_out, hipStream_t s);
};

// ---- the raw frame of one call ----------------------------------------------------------------------------------------
// Where the frame comes from, said once: n rows in host memory; a sageicp_device_frame in the caller's device memory
// (validated by caller_mem.hip), which the ingest kernel reads into d_in on Prep::stream once that stream has waited for the
// caller's; or n records of a sensor_msgs/PointCloud2 payload (sageicp_msg_layout, validated by capi_pipeline.hip) —
// host bytes are uploaded as they are, device bytes are read in place behind the caller's stream — which k_msg_unpack
// (msg.hip) turns into rows.  What follows the load does not know which.
struct FrameSource {
    enum Kind { kHostRows, kDeviceFrame, kMessage };
    Kind kind = kHostRows;
    uint64_t n = 0;
    const double *rows = nullptr;                   // kHostRows: x, y, z, label
    const sageicp_device_frame *frame = nullptr;    // kDeviceFrame
    const unsigned char *payload = nullptr;         // kMessage: n * layout.point_step bytes, in device memory or not
    bool payload_on_device = false;
    sageicp_msg_layout layout{};
    // The pipeline's deskew is on and this call reads the frame's stamps, one per point: `stamps` in host memory (host
    // rows, all finite: checked by the caller), `stamps` in device memory (a device frame), the layout's time field (a
    // message).  Off: the one-argument RegisterFrame, which never deskews; no stamp is read.
    bool read_stamps = false;
    const double *stamps = nullptr;
    hipStream_t stream = nullptr;                   // the caller's: read for device memory only

    static FrameSource host_rows(const double *rows, uint64_t n, bool read_stamps = false, const double *stamps = nullptr) {
        FrameSource s;
        s.n = n; s.rows = rows; s.read_stamps = read_stamps; s.stamps = stamps;
        return s;
    }
    static FrameSource device_frame(const sageicp_device_frame *f, const double *stamps, hipStream_t stream) {
        FrameSource s;
        s.kind = kDeviceFrame; s.n = f->n; s.frame = f; s.stream = stream;
        s.read_stamps = stamps != nullptr; s.stamps = stamps;       // (without stamps it is never deskewed)
        return s;
    }
    static FrameSource message(const void *payload, bool on_device, uint64_t n, const sageicp_msg_layout &layout,
                               bool read_stamps, hipStream_t stream) {
        FrameSource s;
        s.kind = kMessage; s.n = n; s.layout = layout; s.read_stamps = read_stamps; s.stream = stream;
        s.payload = static_cast<const unsigned char *>(payload); s.payload_on_device = on_device;
        return s;
    }
    // an empty message: no rows, no device work
    bool empty_message() const { return kind == kMessage && n == 0; }
    // The stamps go to d_ts with the frame.  Host stamps cross PCIe only when the frame is deskewed (three poses or
    // more); a device frame's and a message's are copied and checked in the load's own pass whenever they are read.
    bool stamps_to_device(bool deskewed) const { return read_stamps && (kind != kHostRows || deskewed); }
};
inline IngestArgs ingest_args(const sageicp_device_frame &f) {
    IngestArgs a{};
    a.xyz = static_cast<const unsigned char *>(f.xyz);
    a.xyz_stride = f.xyz_stride;
    a.xyz_dtype = f.xyz_dtype;
    a.label = static_cast<const unsigned char *>(f.label);
    a.label_stride = f.label_stride;
    a.label_dtype = f.label_dtype;
    a.n = static_cast<int>(f.n);
    return a;
}

// ---- what one Prep::run is asked for ---------------------------------------------------------------------------------
// The levels run in sequence on the device, each feeding the next: level 0 leaves its cloud in d_fd, level 1 in d_src
// (two output buffers: two levels at most).
struct PrepLevel {
    int crop;                           // the range crop of Preprocess() first
    double scale;                       // x the group's voxel size; <= 0: crop only (no voxel test)
};
struct PrepJob {
    double max_range = 0, min_range = 0, label_max_range = 0;
    int n_groups = 0;                   // label groups (8 at most): labels per group, the labels, voxel size per group
    const int *group_counts = nullptr, *group_labels = nullptr;
    const double *group_voxel_size = nullptr;
    int n_levels = 0;
    PrepLevel levels[2] = {};
    // With `dyn` the frame first goes through Preprocess()'s dynamic vehicle filter (dyn_filter.hip), which crops it
    // itself: the levels then start from the filtered cloud with the crop off.
    const DynFilterConfig *dyn = nullptr;
    // With `deskew` the loaded frame is deskewed in place before anything else reads it (the reference's order:
    // DeSkewScan, then Preprocess, then Voxelize; pipeline/sageICP.cpp:36-52).
    // The tangent is (start.inverse() * finish).log() (core/Deskew.cpp:36); the stamps are the FrameSource's.
    const DeskewTangent *deskew = nullptr;
};

// ---- device preprocessing (preprocess.hip): buffers of one pipeline ------------------------------
struct Prep {
    int device = -1;
    OwnedStream stream;
    size_t cap = 0;                     // points the buffers of reserve() hold (all of them: 0 after a failed reserve)
    DevBuf<Point4> d_in, d_tmp, d_fd, d_src;
    DevBuf<uint32_t> d_slot, d_skey, d_sval, d_winner;
    DevBuf<unsigned long long> d_keys;
    DevBuf<unsigned char> d_sort_temp;
    DevBuf<unsigned long long> d_okeys;      // survivors' voxel keys (reference-order emission)
    DevBuf<uint32_t> d_perm;
    PinnedBuf<unsigned long long> h_keys;
    PinnedBuf<uint32_t> h_perm;
    std::vector<uint32_t> h_hash;
    RobinScratch rscratch[8];                // bucket arrays of the order replay, one pair per label group
    std::unique_ptr<ReplayPool> pool;        // parked helper threads of the order replays
    // levels whose survivors are emitted in arrival order even under g_reference_order (bit l): the
    // pipeline's second level — its cloud is only registered, and registration sorts its frame
    // spatially first, so its emission order reaches nothing but the order of fp64 summation
    unsigned arrival_order_levels = 0;
    DevBuf<uint32_t> d_nkept;           // [2]
    DevBuf<int> d_overflow;
    DevBuf<int> d_gcounts, d_glabels;
    PinnedBuf<Point4> h_pin;            // staging for the raw frame and the results
    uint32_t kept_levels[2] = {0, 0};   // points the last run left in d_fd / d_src
    DynFilter dyn;                      // the dynamic vehicle filter's buffers (allocated with its first use)
    bool dyn_ran = false;               // the last run filtered (dyn.info describes its frame)
    // the timestamps of a frame that is deskewed (allocated with the first such frame): pinned staging, device copy
    PinnedBuf<double> h_ts;
    DevBuf<double> d_ts;
    OwnedEvent ev_caller;               // a device frame: orders the caller's stream before `stream` (created with the first)
    // key-frame selection (keyframe.hip): the raw frame copied aside before deskew and the dynamic filter rewrite d_in
    // in place — its coordinates checked — for the pass that follows the registration (allocated with the first use)
    bool keep_raw = false;
    DevBuf<Point4> d_raw;
    // a message's payload (FrameSource::kMessage): pinned staging and device copy of host bytes, the maximum of uint32 stamps
    // (allocated with the first such frame)
    PinnedBuf<unsigned char> h_blob;
    DevBuf<unsigned char> d_blob;
    DevBuf<uint32_t> d_tmax;

    // waits for the stream with the device current, then the members go, dyn's among them: nothing runs on the stream
    // any more (a Prep that never created its stream calls nothing)
    ~Prep();
    int init(int dev);
    // Prepares one frame.  Every level's cloud stays on the device (kept_levels, d_fd / d_src).
    int run(const FrameSource &src, const PrepJob &job);
    // the cloud the last run left at `level`, copied to dst (4 * kept_levels[level] doubles)
    int fetch(int level, double *dst);

private:
    int reserve(size_t n, size_t nlabels);
    int reserve_timestamps(size_t n);
    // the phases of run(), in its order
    int reset_and_reserve(const FrameSource &src, const PrepJob &job);
    int load(const FrameSource &src, bool stamps);
    int ingest(const FrameSource &src, bool stamps);
    int ingest_msg(const FrameSource &src, bool stamps);
    int refuse_bad_timestamp();
    int keep_raw_and_deskew(uint64_t n, const DeskewTangent *deskew);
    int downsample(int level, const Point4 *in, uint64_t n, const PrepJob &job, bool reorder, Point4 *dst, uint32_t &kept);
    int restore_reference_order(int level, Point4 *dst, uint32_t kept);
    int refuse_flags();
};

}  // namespace sageicp
