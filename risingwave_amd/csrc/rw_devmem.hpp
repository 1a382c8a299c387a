// rw_devmem.hpp — the one place device memory is allocated and freed.
//
// The kernel-argument structs (AggTableDev, JoinSideDev, ...) stay plain
// structs of raw pointers; ownership lives beside them in a DevOwner, one
// per executor / caller-owned batch / call. A buffer allocated through an
// owner is freed by release(), by regrow() at the point it is replaced, or
// by the owner's destructor — there is no per-buffer destructor list.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

// bytes currently held by all owners of this library (rw_debug_dev_bytes_live)
inline std::atomic<uint64_t> g_dev_bytes_live{0};

class DevOwner {
    struct Rec {
        void* p;
        size_t bytes;
    };
    std::vector<Rec> recs_;

    void free_rec(size_t i) {
        (void)hipFree(recs_[i].p);
        g_dev_bytes_live -= recs_[i].bytes;
        recs_[i] = recs_.back();
        recs_.pop_back();
    }

public:
    DevOwner() = default;
    DevOwner(const DevOwner&) = delete;
    DevOwner& operator=(const DevOwner&) = delete;
    DevOwner(DevOwner&&) noexcept = default; // the source is left empty
    DevOwner& operator=(DevOwner&&) = delete;
    ~DevOwner() { release_all(); }

    void release_all() {
        while (!recs_.empty()) free_rec(recs_.size() - 1);
    }

    // hipMalloc + record; *slot is nullptr on failure
    template <class T>
    hipError_t alloc(T** slot, size_t bytes) {
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) p = nullptr;
        if (p) {
            recs_.push_back({p, bytes});
            g_dev_bytes_live += bytes;
        }
        *slot = (T*)p;
        return e;
    }

    // alloc sized to a host vector + blocking copy of it (an empty vector
    // yields nullptr); on a failed copy the buffer stays recorded, so the
    // owner still frees it
    template <class T>
    hipError_t upload(T** slot, const std::vector<T>& h) {
        *slot = nullptr;
        if (h.empty()) return hipSuccess;
        size_t bytes = h.size() * sizeof(T);
        hipError_t e = alloc(slot, bytes);
        if (e != hipSuccess) return e;
        return hipMemcpy(*slot, h.data(), bytes, hipMemcpyHostToDevice);
    }

    // free now (hipFree synchronises the device), forget, null the slot
    template <class T>
    void release(T** slot) {
        if (!*slot) return;
        for (size_t i = 0; i < recs_.size(); i++)
            if (recs_[i].p == (void*)*slot) {
                free_rec(i);
                break;
            }
        *slot = nullptr;
    }

    // Replace *slot by a buffer of new_bytes. keep_bytes == 0: free the old
    // one, then allocate (the staging buffers' "free and realloc larger").
    // Otherwise allocate, copy the prefix device-to-device — async on `s`
    // followed by a stream sync when async_copy, a blocking hipMemcpy when
    // not — and free the old buffer right there. On failure *slot keeps
    // what it had (keep_bytes != 0) or is nullptr (keep_bytes == 0).
    template <class T>
    hipError_t regrow(T** slot, size_t new_bytes, size_t keep_bytes = 0,
                      hipStream_t s = nullptr, bool async_copy = false) {
        if (!keep_bytes || !*slot) {
            release(slot);
            return alloc(slot, new_bytes);
        }
        T* np = nullptr;
        hipError_t e = alloc(&np, new_bytes);
        if (e != hipSuccess) return e;
        if (async_copy) {
            e = hipMemcpyAsync(np, *slot, keep_bytes, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
        } else {
            e = hipMemcpy(np, *slot, keep_bytes, hipMemcpyDeviceToDevice);
        }
        if (e != hipSuccess) {
            release(&np);
            return e;
        }
        release(slot);
        *slot = np;
        return hipSuccess;
    }
};

// Kernel timing on an executor's own stream. Event pairs live in a ring and
// are read back lazily — a per-step hipEventSynchronize costs a full host
// round-trip (~45 us, 3x the kernel itself at q7 sizes), so the timed region
// must stay async.
struct EventRing {
    static constexpr int N = 256;
    hipEvent_t ev0[N] = {}, ev1[N] = {};
    uint8_t pending[N] = {};
    uint64_t head = 0;
    double ms_total = 0;

    EventRing() = default;
    EventRing(const EventRing&) = delete;
    EventRing& operator=(const EventRing&) = delete;
    ~EventRing() {
        for (int s = 0; s < N; s++) {
            if (ev0[s]) (void)hipEventDestroy(ev0[s]);
            if (ev1[s]) (void)hipEventDestroy(ev1[s]);
        }
    }

    bool ev_harvest(int slot) {
        if (!pending[slot]) return true;
        float ms = 0;
        if (hipEventSynchronize(ev1[slot]) != hipSuccess ||
            hipEventElapsedTime(&ms, ev0[slot], ev1[slot]) != hipSuccess)
            return false;
        ms_total += ms;
        pending[slot] = 0;
        return true;
    }
    bool harvest_all() {
        for (int s = 0; s < N; s++)
            if (!ev_harvest(s)) return false;
        return true;
    }
    // take a slot, create its pair on first use, reclaim the slot's previous
    // measurement (long complete by the time the ring wraps) without
    // stalling the current step, record ev0. -1 on a HIP error.
    int begin(hipStream_t s) {
        int slot = (int)(head++ % N);
        if (!ev0[slot] && (hipEventCreate(&ev0[slot]) != hipSuccess ||
                           hipEventCreate(&ev1[slot]) != hipSuccess))
            return -1;
        if (!ev_harvest(slot)) return -1;
        return hipEventRecord(ev0[slot], s) == hipSuccess ? slot : -1;
    }
    hipError_t end(int slot, hipStream_t s) {
        hipError_t e = hipEventRecord(ev1[slot], s);
        if (e == hipSuccess) pending[slot] = 1;
        return e;
    }
};
