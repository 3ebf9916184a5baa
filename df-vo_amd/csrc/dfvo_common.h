// Shared internal declarations for libdfvo_hip.so (gfx950 only): errors, the dynamic-LDS attribute, environment switches,
// rounding, streams.  (The convolution interface: conv.h.)
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/dfvo_hip.h"

namespace dfvo {

void set_last_error(const std::string& s);
const char* last_error();

#define DFVO_HIP_CHECK(expr)                                                        \
    do {                                                                            \
        hipError_t _e = (expr);                                                     \
        if (_e != hipSuccess) {                                                     \
            dfvo::set_last_error(std::string(#expr) + ": " + hipGetErrorString(_e)); \
            return DFVO_ERR_HIP;                                                    \
        }                                                                           \
    } while (0)

#define DFVO_ARG_CHECK(cond, msg)                   \
    do {                                            \
        if (!(cond)) {                              \
            dfvo::set_last_error(std::string(msg)); \
            return DFVO_ERR_ARG;                    \
        }                                           \
    } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device function attribute: remembered per (device, kernel) so that a
// process that drives several GPUs (dfvo_set_device) or several pipelines from different threads configures each one
int ensure_dyn_lds(const void* kernel, size_t bytes);

// a DFVO_* on / off switch of the environment: unset = dflt, else whether its integer value is non-zero.  The callers
// read their switch once, into a function-local static.
static inline bool env_flag(const char* name, bool dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) != 0 : dflt;
}

static inline int round_up(int a, int b) { return (a + b - 1) / b * b; }
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Streams of the pipeline are plain non-blocking streams.  Measured dead ends, kept as records only:
// stream priorities for the solver chain (neutral for the chain, -3 .. -9 % for the others: round 2), CU masks that keep a
// few CUs per XCD free of net kernels or confine the solver to them (-10 %: round 2).
static inline hipError_t create_net_stream(hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
static inline hipError_t create_solver_stream(hipStream_t* s, int = 1) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }

// candidate streams classified by the dispatch pipe that serves them (stream_pool.hip)
struct StreamPool {
    std::vector<hipStream_t> s;
    std::vector<int> group;  // pipe group of s[i] (streams of one group slow each other's dispatch), -1 unknown
    int ngroups = 0;         // 0: the probe failed, use creation order
    // hardware queue of s[i]: streams of one queue execute in host enqueue order, whatever their events say (-1 unknown).
    // Streams of one queue are of one pipe group; with fewer hardware queues than candidates several share a queue.
    std::vector<int> queue_group;
    int nqueues = 0;         // 0: the probe failed
    int create(int n);
    hipStream_t take(int group);  // removes a stream of that group from the pool (nullptr when none is left)
    hipStream_t take_index(int i);  // removes candidate i from the pool (nullptr when it was taken before)
    int count(int group) const;
    void release();               // destroys what was not taken
};

}  // namespace dfvo
