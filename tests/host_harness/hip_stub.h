// What the stand-alone lifetime checks share (solver_buffers_check.cpp, net_layers_check.cpp): the few HIP entry points the
// host-only units call, defined on malloc / free, with a "fail the k-th allocation" counter, call counters and a registry of
// the live blocks, streams and events.  Include it in exactly one translation unit of a program.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../df-vo_amd/csrc/dev_mem.h"

using namespace dfvo;

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
            ++g_failed;                                                      \
        }                                                                    \
    } while (0)

// ---- the HIP entry points of the unit under test ----
static std::map<void*, size_t> g_blocks;  // live hipMalloc / hipHostMalloc blocks and their sizes
static std::set<void*> g_streams, g_events;
static int g_allocs = 0, g_frees = 0, g_hip_calls = 0;
static int g_fail_at = -1;  // the allocation (counted from 0 since arm()) that fails; -1: none does
static int g_memsets = 0, g_memset_fail_at = -1;  // the same for hipMemset (counted since arm_memset())
static std::string g_last_error;

static void arm(int fail_at) {
    g_allocs = g_frees = g_hip_calls = 0;
    g_fail_at = fail_at;
}
[[maybe_unused]] static void arm_memset(int fail_at) {
    g_memsets = 0;
    g_memset_fail_at = fail_at;
}
static hipError_t stub_alloc(void** p, size_t bytes) {
    ++g_hip_calls;
    *p = nullptr;
    if (g_allocs++ == g_fail_at) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    g_blocks[*p] = bytes;
    return hipSuccess;
}
static hipError_t stub_free(void* p) {
    ++g_hip_calls;
    ++g_frees;
    if (!p) return hipSuccess;
    CHECK(g_blocks.count(p) == 1);  // a second free of one block, or a pointer that never was one
    if (g_blocks.erase(p)) free(p);
    return hipSuccess;
}
static void* new_handle(std::set<void*>* live) {
    ++g_hip_calls;
    void* h = malloc(1);
    live->insert(h);
    return h;
}
static hipError_t drop_handle(std::set<void*>* live, void* h) {
    ++g_hip_calls;
    CHECK(live->count(h) == 1);  // destroyed twice, or never created
    if (live->erase(h)) free(h);
    return hipSuccess;
}

namespace dfvo {
void set_last_error(const std::string& s) { g_last_error = s; }
const char* last_error() { return g_last_error.c_str(); }
}  // namespace dfvo

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(p, bytes); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return stub_alloc(p, bytes); }
hipError_t hipFree(void* p) { return stub_free(p); }
hipError_t hipHostFree(void* p) { return stub_free(p); }
hipError_t hipMemset(void* p, int v, size_t bytes) {
    ++g_hip_calls;
    auto it = g_blocks.find(p);
    CHECK(it != g_blocks.end() && bytes <= it->second);
    if (it == g_blocks.end() || bytes > it->second) return hipErrorInvalidValue;
    if (g_memsets++ == g_memset_fail_at) return hipErrorUnknown;
    memset(p, v, bytes);
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {  // uploads only
    ++g_hip_calls;
    auto it = g_blocks.find(dst);
    CHECK(kind == hipMemcpyHostToDevice && it != g_blocks.end() && bytes <= it->second);
    if (kind != hipMemcpyHostToDevice || it == g_blocks.end() || bytes > it->second) return hipErrorInvalidValue;
    memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
    *s = (hipStream_t)new_handle(&g_streams);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { return drop_handle(&g_streams, s); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    *e = (hipEvent_t)new_handle(&g_events);
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e) { return drop_handle(&g_events, e); }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) {
    ++g_hip_calls;
    CHECK(g_events.count(e) == 1);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize() {
    ++g_hip_calls;
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stub error"; }
}
