// The archive of a map handle: an append-only log of the voxels the far-voxel sweep evicts, off by
// default.  Each evicted voxel leaves a 32-byte record (its key, its count, where its rows start in the log, the serial
// of the call that evicted it) and its rows, bit for bit in their stored order; calls appear in the order they were
// made, voxels within a call in the order of their eviction (ascending block index; in reference-order mode the order
// the erase-while-iterating sweep erases them).
//
// The older part of the log lives in device memory (d_rows / d_vox, appended to by archive.hip's kernels between the
// search for far voxels and their eviction, on the map's stream), the newest part — evictions that ran on the host copy —
// in a host-side pending tail, which is uploaded behind the device part before anything newer is appended on the device.
// A handle that never touches a device keeps its whole log in the pending tail.
//
// The device append takes no position from an atomic: the counts of the selected voxels are scanned, voxel j's rows
// land at tail + offsets[j], and a one-thread epilogue advances the tail.  With a limit (max_rows) a voxel is archived
// only while all its rows still fit; the end offsets are monotone, so what is kept is a prefix of whole voxels, and the
// first voxel that does not fit makes the archive full for good: from then on evictions are only counted.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "dev_buffer.h"
#include "map_update.h"
#include "sageicp_types.h"

namespace sageicp {

struct ArchiveVoxel {        // sageicp_archive_voxel (include/sageicp.h)
    int32_t x, y, z;
    uint32_t count;
    uint64_t first_row;
    uint64_t update;
};
static_assert(sizeof(ArchiveVoxel) == 32, "the record is 32 bytes");

// the log's counters as the device keeps them: sent before a pass, handed back with the pass's counters (40 bytes, ten of
// h_ctr_aux's sixteen words)
struct ArchiveCtr {
    uint64_t rows, voxels;                   // the tail: rows and records the log holds
    uint64_t dropped_rows, dropped_voxels;   // evicted while full
    uint32_t full, pad;
};
constexpr int kArchiveAuxWord = 2;           // where it sits in MapDevice::h_ctr_aux (word 0: the far voxels found)

// what the append kernels work on
struct ArchiveDev {
    Point4 *rows;
    ArchiveVoxel *vox;
    ArchiveCtr *ctr;
    uint64_t cap_rows, cap_vox;              // what rows / vox hold (nothing is written at or beyond them)
    uint64_t limit_rows;                     // max_rows, or ~0 for none
    uint64_t serial;                         // of this call
    uint32_t *counts, *offsets;              // scratch, [bound + 1] each
    void *temp;
    size_t temp_bytes;
};

size_t archive_temp_bytes(size_t nb);

// The voxels of blocks sel[0 .. *n_sel) (device memory; *n_sel <= bound), still live in M, appended to the log in that
// order; the tail and the dropped counts advanced.  On s; nothing waits.
hipError_t archive_append(const DevMap &M, const ArchiveDev &A, const uint32_t *sel, const uint32_t *n_sel, uint32_t bound,
                          hipStream_t s);

// ---- the selections of an export (LATEST) ----------------------------------------------------------------------------
// scratch of archive_latest for nv records
struct LatestScratch {
    unsigned long long *keys, *keys_alt;     // [nv]
    uint32_t *idx, *idx_alt;                 // [nv]
    uint32_t *flag;                          // [nv]
    uint32_t *sel;                           // [nv] the kept records in log order
    uint32_t *counts, *offsets;              // [nv + 1]
    uint32_t *n_sel;                         // [1]
    void *temp;
    size_t temp_bytes;
};
size_t archive_latest_temp_bytes(size_t nv);
// Record i of vox[0 .. nv) is kept iff no later record has its key and the slot table (table / mask: the map's, in HBM)
// holds no voxel with that key.  The kept records' indices in log order into S.sel, their number into S.n_sel, their
// counts scanned into S.offsets (offsets[*n_sel] == offsets[nv]: the rows of the selection).
hipError_t archive_latest(const ArchiveVoxel *vox, uint32_t nv, const Slot *table, uint32_t mask, const LatestScratch &S,
                          hipStream_t s);
// rows [first, first + n) of the selection S holds, from the log's rows into out[0 .. n)
hipError_t archive_gather_selected(const Point4 *rows, const ArchiveVoxel *vox, const LatestScratch &S, uint64_t first, uint64_t n,
                                   Point4 *out, hipStream_t s);

}  // namespace sageicp

namespace sageicp_impl {
using namespace sageicp;

// The store, one per map handle.
struct MapArchive {
    bool enabled = false, full = false;
    uint64_t max_rows = 0;                   // 0: no limit
    uint64_t updates = 0;                    // eviction-capable calls made while it was on, since it was created or cleared: the next serial
    uint64_t dropped_rows = 0, dropped_voxels = 0;
    // the device part: the first dev_rows rows / dev_vox records of the log
    DevBuf<Point4> d_rows;
    DevBuf<ArchiveVoxel> d_vox;
    DevBuf<ArchiveCtr> d_ctr;
    uint64_t dev_rows = 0, dev_vox = 0;
    // the pending tail: what host-side evictions appended since
    std::vector<Point4> h_rows;
    std::vector<ArchiveVoxel> h_vox;

    uint64_t rows() const { return dev_rows + h_rows.size(); }
    uint64_t voxels() const { return dev_vox + h_vox.size(); }
    uint64_t device_bytes() const {
        return d_rows.capacity() * sizeof(Point4) + d_vox.capacity() * sizeof(ArchiveVoxel) + d_ctr.capacity() * sizeof(ArchiveCtr);
    }
    // a voxel the host copy evicts (before its block is freed), under the limit rule
    void append_host(const int32_t key[3], const Point4 *p, uint32_t count, uint64_t serial);
    // empties the log and releases its device memory; the setting stays
    void clear();
    // ---- the device part (the device current, s a stream of it) ----
    // the pending tail uploaded behind the device part (waits for s only when there is one)
    int flush_pending(hipStream_t s);
    // room for one device update that can evict at most `rows_bound` rows of `vox_bound` voxels; contents kept
    int reserve(uint64_t rows_bound, uint64_t vox_bound, hipStream_t s);
    ArchiveCtr counters() const { return ArchiveCtr{dev_rows, dev_vox, dropped_rows, dropped_voxels, full ? 1u : 0u, 0u}; }
    // what a device update handed back
    void adopt(const ArchiveCtr &c) {
        dev_rows = c.rows;
        dev_vox = c.voxels;
        dropped_rows = c.dropped_rows;
        dropped_voxels = c.dropped_voxels;
        full = c.full != 0;
    }
    // setting and contents of `src`, the device part device to device (nothing runs on src's buffers any more)
    int copy_from(const MapArchive &src, hipStream_t s);
};

}  // namespace sageicp_impl
