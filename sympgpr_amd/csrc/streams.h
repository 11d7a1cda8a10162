// streams.h -- every stream and event the library owns (streams.hip): the pooled events of a factorisation, the per-device
// stream table (panel side stream, the Strassen front end's sum and top streams: strassen.h) and the one release routine.
#pragma once
#include <vector>

#include "common.h"

namespace sgpr {

// Events of one factorisation, BORROWED from a pool the calling thread keeps per device and never gives back.
// Creating and destroying them per call (rounds 1-2) put runtime housekeeping -- event / signal memory being released while
// the device is still running the factorisation that used it -- beside kernels whose workgroups wait for each other; see
// DESIGN 3.9 for what that did to the task-queue driver.  Re-recording an event later is safe: a stream's wait refers to
// the record that was current when the wait was enqueued.  Nested sets (the queue driver, then the look-ahead driver for
// the block it leaves) take consecutive slices of the pool.
struct EventPool {
    std::vector<hipEvent_t> ev;
    size_t top = 0;
};

struct EventSet {
    std::vector<hipEvent_t> ev;
    EventPool *pool = nullptr;
    size_t base = 0;
    int create(size_t count);
    ~EventSet()
    {
        if (pool) pool->top = base;
    }
};
// whatever happens in between, the caller's stream waits for everything queued on the side stream
struct StreamJoin {
    hipStream_t side, caller;
    hipEvent_t ev;
    ~StreamJoin()
    {
        if (hipEventRecord(ev, side) != hipSuccess || hipStreamWaitEvent(caller, ev, 0) != hipSuccess)
            (void)hipStreamSynchronize(side);
        gemm_set_overlap(0);
    }
};

// the high-priority side stream of the device that owns the caller's stream (created on first use, ONE per device)
int side_stream(hipStream_t caller, hipStream_t *out, int *dev_out);
// whoever creates a stream of the library's registers the exit handler that gives them all back
void register_exit_release();
void trim_event_pool();   // the calling thread's pooled events (every device); no factorisation of this thread in flight

// What the release routine does with each handle an owner shows it.  LOOK: is there anything at all; DRAIN: synchronise, then
// destroy, here and now (the owner holds its mutex), the first error kept; AT_EXIT: taken out of the owner's table and
// destroyed afterwards, outside the mutex and without synchronisation.
struct StreamDrop {
    enum Mode { LOOK, DRAIN, AT_EXIT } mode;
    bool any = false;
    hipError_t first = hipSuccess;
    hipStream_t later[12] = {};
    int nlater = 0;
    void stream(hipStream_t &s);
    void event(hipEvent_t &e);   // DRAIN only
};

}  // namespace sgpr
