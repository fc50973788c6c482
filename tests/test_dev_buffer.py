"""The owners of device and pinned memory, of streams and of events (csrc/dev_buffer.h), compiled by g++ against
stand-ins for the HIP calls they make, defined below: every allocation is counted and every call logged, so the order of frees and
allocations, the bytes copied and what is left alive can be checked without a GPU.  A program of its own, not a
library loaded here: in a process that has the HIP runtime loaded, its symbols would take the stand-ins' place.
CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sage-icp_amd", "csrc")

SRC = r'''
#include "dev_buffer.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace sageicp;

namespace {
int live = 0;             // blocks allocated and not yet freed (device and pinned)
int fail_next = 0;        // the next allocation fails
size_t copied = 0;        // bytes of the last copy
std::string trace;        // 'A' allocation, 'F' free, 'C' copy, 'S' synchronisation, 'N' new stream, 'D' stream destroyed,
                          // 'E' event created, 'X' event destroyed, 'V' device made current
int streams = 0, events = 0;   // handles handed out so far: each one is another address
char handles[64];
hipError_t alloc(void **p, size_t bytes) {
    if (fail_next) {
        fail_next = 0;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    ++live;
    trace += 'A';
    return hipSuccess;
}
hipError_t release(void *p) {
    if (p) {
        std::free(p);
        --live;
        trace += 'F';
    }
    return hipSuccess;
}
}  // namespace

hipError_t hipMalloc(void **p, size_t bytes) { return alloc(p, bytes); }
hipError_t hipFree(void *p) { return release(p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return alloc(p, bytes); }
hipError_t hipHostFree(void *p) { return release(p); }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) {
    std::memcpy(dst, src, bytes);
    copied = bytes;
    trace += 'C';
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
    trace += 'S';
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int) {
    *s = reinterpret_cast<hipStream_t>(&handles[streams++]);
    trace += 'N';
    return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int flags, int) { return hipStreamCreateWithFlags(s, flags); }
hipError_t hipExtStreamCreateWithCUMask(hipStream_t *s, uint32_t, const uint32_t *) { return hipStreamCreateWithFlags(s, 0); }
hipError_t hipStreamDestroy(hipStream_t) {
    trace += 'D';
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned int) {
    *e = reinterpret_cast<hipEvent_t>(&handles[32 + events++]);
    trace += 'E';
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t) {
    trace += 'X';
    return hipSuccess;
}
hipError_t hipSetDevice(int) {
    trace += 'V';
    return hipSuccess;
}

#define CHECK(c) do { if (!(c)) return __LINE__; } while (0)

static int destroyed_owners_free_everything() {
    {
        DevBuf<int> d;
        PinnedBuf<double> h;
        PinnedBuf<char, hipHostMallocMapped | hipHostMallocCoherent> mapped;
        CHECK(d.reserve(10) == hipSuccess && h.reserve(3) == hipSuccess && mapped.reserve(7) == hipSuccess);
        CHECK(live == 3 && d.capacity() == 10 && h.capacity() == 3 && mapped.capacity() == 7);
    }
    CHECK(live == 0);
    return 0;
}

static int a_move_hands_over_the_block() {
    {
        DevBuf<int> a;
        CHECK(a.reserve(5) == hipSuccess);
        int *p = a.data();
        DevBuf<int> b(std::move(a));
        CHECK(b.data() == p && b.capacity() == 5 && !a && a.capacity() == 0 && live == 1);
        a.reset();                              // (nothing of its own any more)
        CHECK(live == 1);
    }
    CHECK(live == 0);
    return 0;
}

static int move_assignment_frees_the_old_block() {
    {
        PinnedBuf<int> a, b;
        CHECK(a.reserve(4) == hipSuccess && b.reserve(9) == hipSuccess && live == 2);
        int *p = b.data();
        a = std::move(b);
        CHECK(live == 1 && a.data() == p && a.capacity() == 9 && !b);
    }
    CHECK(live == 0);
    return 0;
}

static int reserve_frees_before_it_allocates() {
    DevBuf<int> d;
    CHECK(d.reserve(4) == hipSuccess);
    trace.clear();
    CHECK(d.reserve(100) == hipSuccess);
    CHECK(trace == "FA" && d.capacity() == 100 && live == 1);
    return 0;
}

static int grow_copies_exactly_keep_elements() {
    DevBuf<int> d;
    CHECK(d.reserve(8) == hipSuccess);
    for (int i = 0; i < 8; ++i) d.data()[i] = 100 + i;
    trace.clear();
    CHECK(d.grow(32, 5, nullptr) == hipSuccess);
    CHECK(trace == "ACSF" && copied == 5 * sizeof(int) && d.capacity() == 32 && live == 1);
    for (int i = 0; i < 5; ++i) CHECK(d.data()[i] == 100 + i);
    // keep beyond what is held: only what is held is copied
    trace.clear();
    CHECK(d.grow(64, 1000, nullptr) == hipSuccess);
    CHECK(trace == "ACSF" && copied == 32 * sizeof(int));
    // nothing to keep: no copy, the same order
    trace.clear();
    CHECK(d.grow(65, 0, nullptr) == hipSuccess);
    CHECK(trace == "ASF" && live == 1);
    return 0;
}

static int a_failed_reserve_leaves_the_owner_empty() {
    PinnedBuf<int> h;
    CHECK(h.reserve(16) == hipSuccess);
    fail_next = 1;
    CHECK(h.reserve(32) == hipErrorOutOfMemory);
    CHECK(!h && h.data() == nullptr && h.capacity() == 0 && live == 0);
    CHECK(h.reserve(2) == hipSuccess && live == 1);
    return 0;
}

static int a_failed_grow_keeps_the_old_block() {
    DevBuf<int> d;
    CHECK(d.reserve(4) == hipSuccess);
    d.data()[3] = 7;
    int *p = d.data();
    fail_next = 1;
    CHECK(d.grow(64, 4, nullptr) == hipErrorOutOfMemory);
    CHECK(d.data() == p && d.capacity() == 4 && d.data()[3] == 7 && live == 1);
    return 0;
}

static int a_stream_owner_waits_then_destroys_before_the_buffers_go() {
    {
        OwnedStream never_created;
        CHECK(never_created.get() == nullptr);
    }
    CHECK(trace.empty());                       // (nothing to wait for or destroy)
    {
        DevBuf<int> d;
        CHECK(d.reserve(4) == hipSuccess);
        OwnedStream s;                          // declared after the buffer: destroyed before it
        CHECK(s.create() == hipSuccess && s.get() != nullptr && trace == "AN");
        trace.clear();
    }
    CHECK(trace == "SDF" && live == 0);
    return 0;
}

static int an_event_owner_destroys_once() {
    {
        OwnedEvent never_created;
        CHECK(!never_created && never_created.get() == nullptr);
    }
    CHECK(trace.empty());
    {
        OwnedEvent timing, ordering;
        CHECK(timing.create(hipEventDefault) == hipSuccess && ordering.create(hipEventDisableTiming) == hipSuccess);
        CHECK(timing && ordering && timing.get() != ordering.get() && trace == "EE");
    }
    CHECK(trace == "EEXX");
    return 0;
}

static int a_moved_stream_owner_is_empty() {
    {
        OwnedStream a;
        CHECK(a.create() == hipSuccess);
        const hipStream_t h = a.get();
        OwnedStream b(std::move(a));
        CHECK(!a && a.get() == nullptr && b && b.get() == h);
        trace.clear();
    }
    CHECK(trace == "SD");
    return 0;
}

static int a_moved_event_owner_is_empty() {
    {
        OwnedEvent a;
        CHECK(a.create(hipEventDisableTiming) == hipSuccess);
        const hipEvent_t h = a.get();
        OwnedEvent b(std::move(a));
        CHECK(!a && a.get() == nullptr && b && b.get() == h);
        trace.clear();
    }
    CHECK(trace == "X");
    return 0;
}

static int move_assignment_releases_the_old_handle_first() {
    {
        OwnedStream a, b;
        CHECK(a.create() == hipSuccess && b.create() == hipSuccess);
        const hipStream_t h = b.get();
        trace.clear();
        a = std::move(b);
        CHECK(trace == "SD" && a.get() == h && !b);     // waited for, then destroyed
        OwnedEvent e, f;
        CHECK(e.create(hipEventDefault) == hipSuccess && f.create(hipEventDefault) == hipSuccess);
        const hipEvent_t g = f.get();
        trace.clear();
        e = std::move(f);
        CHECK(trace == "X" && e.get() == g && !f);
        trace.clear();
    }
    CHECK(trace == "XSD");
    return 0;
}

static int priority_and_masked_streams_go_like_the_plain_one() {
    const uint32_t mask[2] = {0xFFu, 0u};
    {
        DevBuf<int> d;
        CHECK(d.reserve(4) == hipSuccess);
        OwnedStream p;
        CHECK(p.create(-1) == hipSuccess && p && trace == "AN");
        trace.clear();
    }
    CHECK(trace == "SDF");
    trace.clear();
    {
        DevBuf<int> d;
        CHECK(d.reserve(4) == hipSuccess);
        OwnedStream m;
        CHECK(m.create(2, mask) == hipSuccess && m && trace == "AN");
        trace.clear();
    }
    CHECK(trace == "SDF" && live == 0);
    return 0;
}

static int a_growing_vector_of_events_destroys_each_once() {
    {
        std::vector<OwnedEvent> v;                  // (no reserve: it reallocates on the way, as Scratch::events does)
        while (v.size() < 5 * 7) {
            OwnedEvent e;
            CHECK(e.create(hipEventDefault) == hipSuccess);
            v.push_back(std::move(e));
        }
        for (size_t i = 0; i < v.size(); ++i)
            for (size_t j = 0; j < i; ++j) CHECK(v[i] && v[i].get() != v[j].get());
        CHECK(trace == std::string(35, 'E'));       // (nothing destroyed by the moves)
    }
    CHECK(trace == std::string(35, 'E') + std::string(35, 'X'));
    return 0;
}

// the shape of Scratch (capi_internal.h): the first stream declared before the buffers, the second and its event among
// them, the destructor body waiting for both streams with the device current
struct ScratchLike {
    int device = 0;
    OwnedStream stream;
    DevBuf<int> a;
    OwnedStream stream2;
    OwnedEvent ev;
    DevBuf<int> b;
    ~ScratchLike() {
        if (!stream) return;
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream.get());
        if (stream2) (void)hipStreamSynchronize(stream2.get());
    }
};

static int a_handle_waits_for_its_streams_before_anything_goes() {
    { ScratchLike nothing_created; }
    CHECK(trace.empty());
    {
        ScratchLike s;
        CHECK(s.stream.create() == hipSuccess && s.a.reserve(3) == hipSuccess && s.b.reserve(5) == hipSuccess);
        CHECK(s.stream2.create(0) == hipSuccess && s.ev.create(hipEventDisableTiming) == hipSuccess);
        trace.clear();
    }
    // the device, both waits, then the members in reverse order (every stream waited for once more as it goes)
    CHECK(trace == "VSSFXSDFSD");
    const size_t second_wait = trace.find('S', trace.find('S') + 1);
    CHECK(trace[0] == 'V' && second_wait < trace.find('F') && second_wait < trace.find('X') && second_wait < trace.find('D'));
    CHECK(live == 0);
    return 0;
}

// argv[1]: the case; prints the line of the first failed check (0: none), then the blocks still alive
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const std::string c = argv[1];
    int line = -1;
    if (c == "destroyed_owners_free_everything") line = destroyed_owners_free_everything();
    if (c == "a_move_hands_over_the_block") line = a_move_hands_over_the_block();
    if (c == "move_assignment_frees_the_old_block") line = move_assignment_frees_the_old_block();
    if (c == "reserve_frees_before_it_allocates") line = reserve_frees_before_it_allocates();
    if (c == "grow_copies_exactly_keep_elements") line = grow_copies_exactly_keep_elements();
    if (c == "a_failed_reserve_leaves_the_owner_empty") line = a_failed_reserve_leaves_the_owner_empty();
    if (c == "a_failed_grow_keeps_the_old_block") line = a_failed_grow_keeps_the_old_block();
    if (c == "a_stream_owner_waits_then_destroys_before_the_buffers_go")
        line = a_stream_owner_waits_then_destroys_before_the_buffers_go();
    if (c == "an_event_owner_destroys_once") line = an_event_owner_destroys_once();
    if (c == "a_moved_stream_owner_is_empty") line = a_moved_stream_owner_is_empty();
    if (c == "a_moved_event_owner_is_empty") line = a_moved_event_owner_is_empty();
    if (c == "move_assignment_releases_the_old_handle_first") line = move_assignment_releases_the_old_handle_first();
    if (c == "priority_and_masked_streams_go_like_the_plain_one") line = priority_and_masked_streams_go_like_the_plain_one();
    if (c == "a_growing_vector_of_events_destroys_each_once") line = a_growing_vector_of_events_destroys_each_once();
    if (c == "a_handle_waits_for_its_streams_before_anything_goes") line = a_handle_waits_for_its_streams_before_anything_goes();
    std::printf("%d %d\n", line, live);
    return 0;
}
'''

CASES = ["destroyed_owners_free_everything", "a_move_hands_over_the_block", "move_assignment_frees_the_old_block",
         "reserve_frees_before_it_allocates", "grow_copies_exactly_keep_elements",
         "a_failed_reserve_leaves_the_owner_empty", "a_failed_grow_keeps_the_old_block",
         "a_stream_owner_waits_then_destroys_before_the_buffers_go",
         "an_event_owner_destroys_once", "a_moved_stream_owner_is_empty", "a_moved_event_owner_is_empty",
         "move_assignment_releases_the_old_handle_first", "priority_and_masked_streams_go_like_the_plain_one",
         "a_growing_vector_of_events_destroys_each_once", "a_handle_waits_for_its_streams_before_anything_goes"]


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile dev_buffer.h for the host")
    d = tmp_path_factory.mktemp("devbuf")
    src, out = d / "devbuf.cpp", d / "devbuf"
    src.write_text(SRC)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-deprecated-declarations",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, str(src), "-o", str(out)])
    return str(out)


@pytest.mark.parametrize("case", CASES)
def test_dev_buffer(prog, case):
    line, live = map(int, subprocess.check_output([prog, case], text=True).split())
    assert line == 0, "check failed at line %d of the test's C++ source" % line
    # every case ends with its owners destroyed
    assert live == 0
