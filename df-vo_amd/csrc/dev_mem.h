// Move-only owners of one hipMalloc (DevArr) or hipHostMalloc (PinnedArr) block.  Host code only.
// The one failure rule of every buffer set built from them: `n` never exceeds what `p` holds, whether a call succeeded or
// failed.  No object with static storage duration may hold one (its destructor would call HIP behind the runtime's own).
#pragma once
#include <utility>

#include "dfvo_common.h"

namespace dfvo {

template <class T, bool PINNED>
struct HipArr {
    T* p = nullptr;
    size_t n = 0;  // elements
    HipArr() = default;
    HipArr(HipArr&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    HipArr& operator=(HipArr&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p, n = o.n;
            o.p = nullptr, o.n = 0;
        }
        return *this;
    }
    ~HipArr() { release(); }
    operator T*() const { return p; }
    // releases what it holds, then allocates `count` elements; on failure the array is empty
    int alloc(size_t count) {
        release();
        void* q = nullptr;
        if (PINNED)
            DFVO_HIP_CHECK(hipHostMalloc(&q, sizeof(T) * count, hipHostMallocDefault));
        else
            DFVO_HIP_CHECK(hipMalloc(&q, sizeof(T) * count));
        p = (T*)q, n = count;
        return DFVO_OK;
    }
    // alloc, then a synchronous zero fill; the array is empty if either fails
    int alloc_zeroed(size_t count) {
        const int rc = alloc(count);
        if (rc != DFVO_OK) return rc;
        HipArr filled(std::move(*this));  // released on the early return below
        DFVO_HIP_CHECK(hipMemset(filled.p, 0, sizeof(T) * count));
        *this = std::move(filled);
        return DFVO_OK;
    }
    // no HIP call when `count` elements fit
    int grow(size_t count) { return count <= n ? DFVO_OK : alloc(count); }
    void release() {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr, n = 0;
    }
    // hands the block to the caller (who frees it); the array is empty afterwards
    T* detach() {
        T* q = p;
        p = nullptr, n = 0;
        return q;
    }
};
template <class T>
using DevArr = HipArr<T, false>;
template <class T>
using PinnedArr = HipArr<T, true>;

}  // namespace dfvo
