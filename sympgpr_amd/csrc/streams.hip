// streams.hip -- the streams and events libsympgpr_hip.so creates, and the one routine that gives them back (streams.h).
#include <cstdlib>
#include <mutex>

#include "cholq.h"
#include "strassen.h"
#include "streams.h"

namespace sgpr {

namespace {

thread_local EventPool t_event_pool[MAX_DEVICES];

// The high-priority side stream of the device that owns the caller's stream (created on first use, ONE per device,
// shared by every handle and every host thread; release_device() gives it back).
//
// Forward progress with several handles factoring at once: every panel_kernel of a device is launched on this one
// in-order stream, so at most one panel kernel -- one set of spinning strips -- is resident per device at any time,
// whatever number of handles / threads are factoring.  The workgroups it waits for are its own (dispatched in block
// order, each as soon as ONE CU drains); everything else on the device is an MFMA / Gram / solve launch whose
// workgroups end by themselves.  tests/test_gpu_stress.py runs three handles at n = 16384 against this.
// The library's streams on one device, created on first use.  Slot 0: that side stream, at the HIGHEST priority.  Slots 1, 2: the
// Strassen front end's operand sums (strassen.hip: run_schedule), at the LOWEST -- the sums fill what the products leave free and
// must never hold one up.  Slot 3: the passes of the top Strassen level (run_top), lowest too and a stream of their own, because
// run_schedule makes its side stream wait for the caller's at every entry -- a top pass queued there would sit in front of the
// next half-size call's first inner sums.  Caller + panel + sums + top passes: four hardware queues.
enum { SLOT_PANEL = 0, SLOT_SUM = 1, SLOT_TOP = 3, N_SLOT = 4 };
hipStream_t g_streams[MAX_DEVICES][N_SLOT] = {};
std::mutex g_side_mu;                                      // two fit handles may factor for the first time at once

// out[0 .. count): the streams of slots first .. first + count - 1 on the device that owns the caller's stream (the null stream
// belongs to the current device); bad_device: the message for a device index out of range
int lib_streams(hipStream_t caller, int first, int count, const char *bad_device, hipStream_t *out, int *dev_out = nullptr)
{
    hipError_t e = hipSuccess;
    const int dev = device_of(caller, &e);
    SGPR_HIP(e);
    if (dev < 0 || !out || count < 1) { set_error(bad_device); return SGPR_E_ARG; }
    std::lock_guard<std::mutex> lock(g_side_mu);
    for (int slot = first; slot < first + count; ++slot) {
        hipStream_t &s = g_streams[dev][slot];
        if (!s) {
            int cur = -1, lo = 0, hi = 0;
            SGPR_HIP(hipGetDevice(&cur));
            if (cur != dev) SGPR_HIP(hipSetDevice(dev));
            e = hipDeviceGetStreamPriorityRange(&lo, &hi);
            if (e == hipSuccess) e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, slot == SLOT_PANEL ? hi : lo);
            if (e == hipSuccess) register_exit_release();
            if (cur != dev) (void)hipSetDevice(cur);
            SGPR_HIP(e);
        }
        out[slot - first] = s;
    }
    if (dev_out) *dev_out = dev;
    return 0;
}

// Every stream of the library on `dev`, shown to `d` by its owner under the owner's mutex: the slot table here, the task-queue
// driver's masked pairs (and its own state) in cholq.hip.
void walk_streams(int dev, StreamDrop &d)
{
    {
        std::lock_guard<std::mutex> lock(g_side_mu);
        for (hipStream_t &s : g_streams[dev]) d.stream(s);
    }
    cholq::queue_release(dev, d);
}

// drain: synchronise and destroy the streams this library created on `dev` (side stream, sum / top streams, the queue driver's
// masked pairs and its event); the next factorisation creates them again.  The caller guarantees no factorisation is being
// enqueued.  Not drain (the exit handler): no synchronisation -- a stream that is still busy is released when its work ends.
int release_streams(int dev, bool drain)
{
    int cur = -1;
    if (drain) {
        // nothing of ours on this device: do not even touch it (an exit hook calls this for every device of the box)
        StreamDrop look{StreamDrop::LOOK};
        walk_streams(dev, look);
        if (!look.any) return 0;
        SGPR_HIP(hipGetDevice(&cur));
        if (cur != dev) SGPR_HIP(hipSetDevice(dev));
        StreamDrop d{StreamDrop::DRAIN};
        walk_streams(dev, d);
        if (cur != dev) (void)hipSetDevice(cur);
        SGPR_HIP(d.first);
        return 0;
    }
    StreamDrop d{StreamDrop::AT_EXIT};
    walk_streams(dev, d);
    if (!d.nlater) return 0;
    (void)hipGetDevice(&cur);
    if (cur != dev) (void)hipSetDevice(dev);
    for (int q = 0; q < d.nlater; ++q) (void)hipStreamDestroy(d.later[q]);
    if (cur != dev && cur >= 0) (void)hipSetDevice(cur);
    return 0;
}

// The streams this library creates are handed back by an exit handler of the LIBRARY, registered when the first of them is
// created: atexit handlers run in reverse order of registration, the HIP runtime registered its own when it was initialised
// (before any stream could exist), so this one runs while the runtime is still whole.  Round 3 did this from the Python
// binding only (a run under rocprofv3 --kernel-trace that had used the CU-masked streams crashed in an exit handler when
// they were left to the runtime's own teardown); users of the C ABI get the same now.  No synchronisation here: a stream
// that is still busy is released when its work ends.
void release_all_streams_at_exit()
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); return; }
    for (int dev = 0; dev < ndev && dev < MAX_DEVICES; ++dev) (void)release_streams(dev, false);
    (void)hipGetLastError();
}

}  // namespace

void StreamDrop::stream(hipStream_t &s)
{
    if (!s) return;
    any = true;
    if (mode == LOOK) return;
    if (mode == DRAIN) {
        hipError_t e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = hipStreamDestroy(s);
        if (e != hipSuccess && first == hipSuccess) first = e;
    } else {
        later[nlater++] = s;
    }
    s = nullptr;
}

void StreamDrop::event(hipEvent_t &e)
{
    if (!e) return;
    const hipError_t r = hipEventDestroy(e);
    if (r != hipSuccess && first == hipSuccess) first = r;
    e = nullptr;
}

int EventSet::create(size_t count)
{
    int dev = 0;
    SGPR_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) { set_error("potrf: device index out of range"); return SGPR_E_ARG; }
    pool = &t_event_pool[dev];
    base = pool->top;
    while (pool->ev.size() < base + count) {
        hipEvent_t e = nullptr;
        SGPR_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        pool->ev.push_back(e);
    }
    pool->top = base + count;
    ev.assign(pool->ev.begin() + (long)base, pool->ev.begin() + (long)(base + count));
    return 0;
}

void trim_event_pool()
{
    for (int dev = 0; dev < MAX_DEVICES; ++dev) {
        EventPool &p = t_event_pool[dev];
        if (p.ev.empty() || p.top != 0) continue;
        for (hipEvent_t e : p.ev) (void)hipEventDestroy(e);
        p.ev.clear();
    }
    (void)hipGetLastError();
}

void register_exit_release()
{
    static std::once_flag once;
    std::call_once(once, [] { (void)atexit(release_all_streams_at_exit); });
}

int side_stream(hipStream_t caller, hipStream_t *out, int *dev_out) { return lib_streams(caller, SLOT_PANEL, 1, "potrf: device index out of range", out, dev_out); }

int strassen_sum_streams(hipStream_t caller, int count, hipStream_t *out)
{
    return lib_streams(caller, SLOT_SUM, (count == 1 || count == 2) ? count : 0, "strassen_sum_streams: bad device or count", out);
}
int strassen_top_stream(hipStream_t caller, hipStream_t *out) { return lib_streams(caller, SLOT_TOP, 1, "strassen_top_stream: bad device", out); }

int release_device_streams(int dev)
{
    if (dev < 0 || dev >= MAX_DEVICES) { set_error("release_device_streams: device index out of range"); return SGPR_E_ARG; }
    return release_streams(dev, true);
}

}  // namespace sgpr
